// Per-item logic of the numeric categories (reference: cpp/src/category/numeric_category.inl).  Shared by the kernels of
// cs_numcat.hip and the g++ harness of tests/test_numcat_cpu.py; tests/numcat_model.py restates it independently.
//
// A number of type int8 / int32 / int64 / float32 / float64 has an IMAGE in a uint64_t:
//   order     image(a) < image(b) exactly when a < b -- signed integers are sign-biased, floats get the usual flip
//             (negative -> ~bits, otherwise bits | sign).  The 8- and 32-bit types sit in the low bits, the upper bytes are
//             zero (the radix sort skips a digit that is the same everywhere).
//   equality  image(a) == image(b) exactly when a == b: -0.0 and +0.0 share the image of +0.0.  NaN != NaN has no place in
//             a key set: every NaN has one image, the largest of its type (it sorts behind +inf).
// Integers come back from their image exactly.  A float class with more than one member (the zeros, the NaNs) comes back
// as +0.0 / the quiet NaN; the kernels put the number of the class's lowest-indexed row in its place.
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define CSNUM_HD __host__ __device__ __forceinline__
#else
#define CSNUM_HD inline
#endif

namespace csnum {

enum Type { T_I8 = 0, T_I32 = 1, T_I64 = 2, T_F32 = 3, T_F64 = 4 };  // cs_numtype

constexpr uint64_t kZero32 = 0x80000000ull, kNan32 = 0xFFC00000ull, kInf32 = 0xFF800000ull;
constexpr uint64_t kZero64 = 0x8000000000000000ull, kNan64 = 0xFFF8000000000000ull, kInf64 = 0xFFF0000000000000ull;

template <class T>
struct Image;

template <>
struct Image<int8_t> {
  static constexpr int type = T_I8;
  static constexpr bool classes = false;  // no image has more than one number
  static CSNUM_HD uint64_t of(int8_t v) { return (uint64_t)((uint8_t)v ^ 0x80u); }
  static CSNUM_HD int8_t back(uint64_t m) { return (int8_t)((uint8_t)m ^ 0x80u); }
};
template <>
struct Image<int32_t> {
  static constexpr int type = T_I32;
  static constexpr bool classes = false;
  static CSNUM_HD uint64_t of(int32_t v) { return (uint64_t)((uint32_t)v ^ 0x80000000u); }
  static CSNUM_HD int32_t back(uint64_t m) { return (int32_t)((uint32_t)m ^ 0x80000000u); }
};
template <>
struct Image<int64_t> {
  static constexpr int type = T_I64;
  static constexpr bool classes = false;
  static CSNUM_HD uint64_t of(int64_t v) { return (uint64_t)v ^ kZero64; }
  static CSNUM_HD int64_t back(uint64_t m) { return (int64_t)(m ^ kZero64); }
};
template <>
struct Image<float> {
  static constexpr int type = T_F32;
  static constexpr bool classes = true;
  static constexpr uint64_t zero = kZero32, nan = kNan32;
  static CSNUM_HD uint64_t of(float v) {
    uint32_t b;
    memcpy(&b, &v, 4);
    if ((b & 0x7FFFFFFFu) > 0x7F800000u) return kNan32;
    if ((b & 0x7FFFFFFFu) == 0) return kZero32;
    return (uint64_t)((b & 0x80000000u) ? ~b : (b | 0x80000000u));
  }
  static CSNUM_HD float back(uint64_t m) {
    const uint32_t i = (uint32_t)m;
    uint32_t b = i == (uint32_t)kNan32 ? 0x7FC00000u : (i & 0x80000000u) ? (i & 0x7FFFFFFFu) : ~i;
    float v;
    memcpy(&v, &b, 4);
    return v;
  }
};
template <>
struct Image<double> {
  static constexpr int type = T_F64;
  static constexpr bool classes = true;
  static constexpr uint64_t zero = kZero64, nan = kNan64;
  static CSNUM_HD uint64_t of(double v) {
    uint64_t b;
    memcpy(&b, &v, 8);
    if ((b & ~kZero64) > 0x7FF0000000000000ull) return kNan64;
    if ((b & ~kZero64) == 0) return kZero64;
    return (b & kZero64) ? ~b : (b | kZero64);
  }
  static CSNUM_HD double back(uint64_t m) {
    uint64_t b = m == kNan64 ? 0x7FF8000000000000ull : (m & kZero64) ? (m & ~kZero64) : ~m;
    double v;
    memcpy(&v, &b, 8);
    return v;
  }
};

// the caller's bitmask: LSB first, a 0 bit is a null item; no bitmask, no nulls
CSNUM_HD bool is_null(const uint8_t* nulls, int64_t i) { return nulls && ((nulls[i >> 3] >> (i & 7)) & 1u) == 0; }

// 64-bit mix (the finalizer of MurmurHash3): where an image starts probing in the table
CSNUM_HD uint64_t mix(uint64_t k) {
  k ^= k >> 33;
  k *= 0xff51afd7ed558ccdull;
  k ^= k >> 33;
  k *= 0xc4ceb9fe1a85ec53ull;
  k ^= k >> 33;
  return k;
}

inline int type_bytes(int type) { return type == T_I8 ? 1 : (type == T_I32 || type == T_F32) ? 4 : 8; }

}  // namespace csnum
