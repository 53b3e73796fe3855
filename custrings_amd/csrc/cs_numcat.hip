// Numeric categories (reference: cpp/src/category/numeric_category.inl): sorted unique keys of int8 / int32 / int64 /
// float32 / float64 and one int32 value per row.  Everything works on the order-preserving 64-bit IMAGE of a number
// (numcat_ops.h), so one set of kernels serves the five types and the sort is cs_radix.hip's.
//
//   build     every non-null row's image goes into an open-addressing table of 64-bit slots (k_insert: read the slot, CAS
//             only an empty one); the row that fills a slot appends (image, slot) to the list of distinct keys.  Only that
//             list is sorted (radix_sort_pairs64); a key's slot then takes its rank; values[row] = rank in the slot the row found.
//             The reference sorts all N rows with a comparator (numeric_category.inl:196-225).
//   key sets  add / remove / set keys and merge: the images of (old keys ++ new items), with their positions, go through the
//             STABLE radix sort; a key is then the head of a run of equal images, old before new, and "is it in both sets"
//             is a look at the neighbour (the reference's stable_sort_by_key + unique, .inl:487-870).  The int32 side --
//             remap, mark-used, compact -- is cat_remap.h, shared with the string categories.
//
// One invariant: a row is null exactly when the key set includes the null key (key 0) and the row's value is 0.  The
// bitmask is therefore a function of the values and is made by one kernel (k_mask) wherever a category is finished.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <memory>

#include "cat_remap.h"
#include "cs_internal.h"
#include "device_utils.h"
#include "numcat_ops.h"

using namespace cs;
using namespace csdev;
using csnum::Image;

struct cs_numcat {
  int type = 0;
  int64_t rows = 0, nkeys = 0;
  bool keys_have_null = false;
  int64_t null_rows = 0;
  Buf keys;    // T[nkeys]; with keys_have_null key 0 is the null key (its number: the lowest-indexed null row's)
  Buf values;  // int32[rows]
  Buf nulls;   // uint8[(rows + 7) / 8], LSB first, 0 = null; absent unless keys_have_null
};

namespace {

constexpr uint64_t kEmpty = ~0ull;  // an empty slot; the one image with this value (int64 max) is carried by a flag instead
constexpr int32_t kRowNull = -1, kRowMax = -2;

struct BuildFlags {  // filled by k_insert, read by the host
  unsigned long long distinct;
  int32_t first_null, first_zero, first_nan;
  unsigned saw_max;
};

// the lowest row of the wave for which `c` holds lowers *at (rows ascend with the lane)
__device__ __forceinline__ void wave_min_row(bool c, int64_t i, int32_t* at) {
  const unsigned long long m = __ballot(c);
  if (c && (m & ((1ull << (threadIdx.x & 63)) - 1ull)) == 0) atomicMin(at, (int32_t)i);
}

template <class T>
__global__ void __launch_bounds__(kBlock) k_insert(const T* __restrict__ items, const uint8_t* __restrict__ nulls, int64_t n, unsigned long long* table,
                                                   uint64_t slot_mask, uint64_t* __restrict__ dk, int32_t* __restrict__ ds, BuildFlags* flags,
                                                   int32_t* __restrict__ values) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const bool active = i < n;
  const bool null = active && csnum::is_null(nulls, i);
  const bool live = active && !null;
  const uint64_t img = live ? Image<T>::of(items[i]) : 0;
  wave_min_row(null, i, &flags->first_null);
  if constexpr (Image<T>::classes) {
    wave_min_row(live && img == Image<T>::zero, i, &flags->first_zero);
    wave_min_row(live && img == Image<T>::nan, i, &flags->first_nan);
  }
  if (!active) return;
  if (null) {
    values[i] = kRowNull;
    return;
  }
  if (img == kEmpty) {
    flags->saw_max = 1u;  // (every writer writes the same word)
    values[i] = kRowMax;
    return;
  }
  uint64_t h = csnum::mix(img) & slot_mask;
  for (;;) {  // ends: the table has more slots than the column has rows
    unsigned long long cur = __hip_atomic_load(table + h, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (cur == kEmpty) {
      cur = atomicCAS(table + h, (unsigned long long)kEmpty, (unsigned long long)img);
      if (cur == kEmpty) {
        // (one address, the constant 1: the compiler's atomic optimizer makes this one atomic per wave -- the lanes that won
        // a slot in this round are counted with a ballot and offset by their rank among them)
        const unsigned long long at = atomicAdd(&flags->distinct, 1ull);
        dk[at] = img;
        ds[at] = (int32_t)h;
        break;
      }
    }
    if (cur == img) break;
    h = (h + 1) & slot_mask;
  }
  values[i] = (int32_t)h;
}

// the number a key's image stands for: the lowest-indexed row of a class with several members, else the image's own
template <class T>
__device__ __forceinline__ T number_of(uint64_t img, const T* __restrict__ items, int32_t first_zero, int32_t first_nan) {
  if constexpr (Image<T>::classes) {
    if (img == Image<T>::zero && first_zero >= 0) return items[first_zero];
    if (img == Image<T>::nan && first_nan >= 0) return items[first_nan];
  }
  return Image<T>::back(img);
}
template <class T>
__global__ void k_rank(const uint64_t* __restrict__ dk, const int32_t* __restrict__ ds, int64_t k, int32_t base, const T* __restrict__ items,
                       int32_t first_null, int32_t first_zero, int32_t first_nan, unsigned long long* __restrict__ table, T* __restrict__ keys) {
  const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (j == 0 && base) keys[0] = items[first_null];
  if (j >= k) return;
  const int32_t slot = ds[j];
  if (slot >= 0) table[slot] = (unsigned long long)j;  // the slot's image has done its work: the slot now holds the key's rank
  keys[base + j] = number_of<T>(dk[j], items, first_zero, first_nan);
}
__global__ void k_values(int32_t* __restrict__ values, int64_t n, const unsigned long long* __restrict__ table, int32_t base, int32_t last) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const int32_t v = values[i];
  values[i] = v == kRowNull ? 0 : v == kRowMax ? last : base + (int32_t)table[v];
}
// the image no slot can hold joins the distinct keys (it is the largest there is, so it sorts last)
__global__ void k_append_max(uint64_t* __restrict__ dk, int32_t* __restrict__ ds, int64_t at) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    dk[at] = kEmpty;
    ds[at] = -1;
  }
}
// *bad |= 1 when a position lies outside [0, limit)
__global__ void k_check_range(const int32_t* __restrict__ pos, int64_t n, int64_t limit, unsigned* __restrict__ bad) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const bool oob = i < n && (pos[i] < 0 || pos[i] >= limit);
  if (__any(oob) && (threadIdx.x & 63) == 0) atomicOr(bad, 1u);
}

// bitmask byte b: bit r = !(have_null && values[8 b + r] == 0), rows beyond n are 0 bits; *null_rows counts the 0 bits within n
__global__ void k_mask(const int32_t* __restrict__ values, int64_t n, int have_null, uint8_t* __restrict__ mask, unsigned long long* null_rows) {
  const int64_t b = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  int zeros = 0;
  if (b * 8 < n) {
    unsigned m = 0;
    for (int r = 0; r < 8; ++r) {
      const int64_t i = b * 8 + r;
      if (i >= n) break;
      const bool null = have_null && values[i] == 0;
      m |= (null ? 0u : 1u) << r;
      zeros += null;
    }
    mask[b] = (uint8_t)m;
  }
  if (null_rows) {
    zeros = wave_reduce_sum(zeros);
    if ((threadIdx.x & 63) == 0 && zeros) atomicAdd(null_rows, (unsigned long long)zeros);
  }
}

template <class T>
__global__ void k_to_type(const T* __restrict__ keys, int64_t nkeys, const int32_t* __restrict__ values, int64_t n, T* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const int32_t v = values[i];
  out[i] = (v >= 0 && v < nkeys) ? keys[v] : T(0);  // (a value of -1 -- its key was removed -- reads as 0)
}
__global__ void k_gather_values(const int32_t* __restrict__ values, int64_t rows, const int32_t* __restrict__ pos, int64_t n, int32_t* __restrict__ out,
                                unsigned* __restrict__ bad) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  bool oob = false;
  if (i < n) {
    const int32_t p = pos[i];
    oob = p < 0 || p >= rows;
    out[i] = oob ? -1 : values[p];
  }
  if (__any(oob) && (threadIdx.x & 63) == 0) atomicOr(bad, 1u);
}
__global__ void k_count_equal(const int32_t* __restrict__ values, int64_t n, int32_t want, unsigned long long* __restrict__ count) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const int hits = wave_reduce_sum(i < n && values[i] == want ? 1 : 0);
  if ((threadIdx.x & 63) == 0 && hits) atomicAdd(count, (unsigned long long)hits);
}
__global__ void k_flag_equal(const int32_t* __restrict__ values, int64_t n, int32_t want, int32_t* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i < n) out[i] = values[i] == want ? 1 : 0;
}
template <class T>
__global__ void k_find(const T* __restrict__ keys, int64_t k, int32_t base, uint64_t img, int32_t* __restrict__ out) {
  const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (j < k && Image<T>::of(keys[j]) == img) *out = base + (int32_t)j;  // (the keys are distinct: one writer at the most)
}

// ---- key sets ----------------------------------------------------------------------------------------------------------
__global__ void k_flag_valid(const uint8_t* __restrict__ nulls, int64_t n, int32_t* __restrict__ flags, int32_t* first_null) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const bool null = i < n && csnum::is_null(nulls, i);
  wave_min_row(null, i, first_null);
  if (i < n) flags[i] = null ? 0 : 1;
}
// img / idx [at + t] = the image of src[pos ? pos[t] : t] and that position counted from `at0`
template <class T>
__global__ void k_images(const T* __restrict__ src, const int32_t* __restrict__ pos, int64_t n, int64_t at, int32_t at0, uint64_t* __restrict__ img,
                         int32_t* __restrict__ idx) {
  const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (t >= n) return;
  const int32_t p = pos ? pos[t] : (int32_t)t;
  img[at + t] = Image<T>::of(src[p]);
  idx[at + t] = at0 + p;
}
enum SetOp { OP_ADD = 0, OP_REMOVE = 1, OP_SET = 2 };
// over the sorted pairs: flags[j] = 1 where j heads a run of equal images that the operation keeps as a key
__global__ void k_heads(const uint64_t* __restrict__ img, const int32_t* __restrict__ idx, int64_t n, int32_t ko, int op, int32_t* __restrict__ flags) {
  const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (j >= n) return;
  const uint64_t m = img[j];
  const bool head = j == 0 || img[j - 1] != m;
  const bool is_old = idx[j] < ko;  // (the old keys are distinct and sort first within a run: an old key is always a head)
  const bool has_new = !is_old || (j + 1 < n && img[j + 1] == m);
  flags[j] = head && (op == OP_ADD || (op == OP_REMOVE ? (is_old && !has_new) : has_new));
}
// keys[base + slot] = the number of every kept head; table[hn + old key] = its new index or -1; with table2 (merge: every
// run is kept, the items are distinct) table2[hn2 + item] = the index of the item's run
template <class T>
__global__ void k_emit(const int32_t* __restrict__ idx, const int32_t* __restrict__ flags, const int64_t* __restrict__ slot, int64_t n, int32_t ko,
                       const T* __restrict__ old_keys, const T* __restrict__ items, int32_t base, T* __restrict__ keys, int32_t* __restrict__ table,
                       int32_t* __restrict__ table2) {
  const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (j >= n) return;
  const int32_t p = idx[j];
  const bool keep = flags[j] != 0, is_old = p < ko;
  const int32_t at = base + (int32_t)slot[j];
  if (keep) keys[at] = is_old ? old_keys[p] : items[p - ko];
  if (is_old) table[p] = keep ? at : -1;
  else if (table2) table2[p - ko] = keep ? at : at - 1;
}
template <class T>
__global__ void k_copy_one(const T* __restrict__ from, T* __restrict__ to) {
  if (threadIdx.x == 0 && blockIdx.x == 0) *to = *from;
}
template <class T>
__global__ void k_gather_keys(const T* __restrict__ keys, const int32_t* __restrict__ pos, int64_t n, T* __restrict__ out) {
  const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (t < n) out[t] = keys[pos[t]];
}

template <class F>
void dispatch(int type, F&& f) {
  switch (type) {
    case CS_NUM_I8: return f(int8_t());
    case CS_NUM_I32: return f(int32_t());
    case CS_NUM_I64: return f(int64_t());
    case CS_NUM_F32: return f(float());
    case CS_NUM_F64: return f(double());
  }
  fail(CS_ERR_INVALID_ARG, "numeric category: unknown type");
}
size_t at_least(size_t bytes) { return bytes ? bytes : 1; }

// the bitmask and the null-row count from the values (the invariant), then the stream is waited for
cs_numcat* finish(std::unique_ptr<cs_numcat> c, hipStream_t s) {
  c->nulls.reset();
  c->null_rows = 0;
  if (c->keys_have_null && c->rows) {
    const int64_t nb = (c->rows + 7) / 8;
    c->nulls = dev_alloc(nb, s);
    Buf cnt = zeroed_count(s);
    hipLaunchKernelGGL(k_mask, dim3(blocks_for(nb)), dim3(kBlock), 0, s, ptr<const int32_t>(c->values), c->rows, 1, ptr<uint8_t>(c->nulls),
                       ptr<unsigned long long>(cnt));
    c->null_rows = read_count(cnt, s);
  }
  CS_HIP(hipGetLastError());
  CS_HIP(hipStreamSynchronize(s));
  return c.release();
}
std::unique_ptr<cs_numcat> blank(int type, int64_t rows, int64_t nkeys, bool have_null, hipStream_t s) {
  auto c = std::make_unique<cs_numcat>();
  c->type = type;
  c->rows = rows;
  c->nkeys = nkeys;
  c->keys_have_null = have_null;
  c->keys = dev_alloc(at_least((size_t)nkeys * csnum::type_bytes(type)), s);
  c->values = dev_alloc(at_least(sizeof(int32_t) * (size_t)rows), s);
  return c;
}
// the same keys (shared: buffers are immutable) over other values
std::unique_ptr<cs_numcat> same_keys(const cs_numcat* cat, int64_t rows, hipStream_t s) {
  auto c = std::make_unique<cs_numcat>();
  c->type = cat->type;
  c->rows = rows;
  c->nkeys = cat->nkeys;
  c->keys_have_null = cat->keys_have_null;
  c->keys = cat->keys;
  c->values = dev_alloc(at_least(sizeof(int32_t) * (size_t)rows), s);
  return c;
}

template <class T>
cs_numcat* build(const T* items, int64_t n, const uint8_t* nulls, hipStream_t s) {
  const int type = Image<T>::type;
  if (!items || n == 0) return finish(blank(type, 0, 0, false, s), s);  // .inl:201-202: an empty category
  uint64_t slots = 1024;
  while (slots < 2 * (uint64_t)n && slots < (1ull << 31)) slots <<= 1;  // more slots than rows; slot ids travel as int32
  Buf table = dev_alloc(sizeof(uint64_t) * slots, s);
  CS_HIP(hipMemsetAsync(table->p, 0xFF, sizeof(uint64_t) * slots, s));
  Buf dk = dev_alloc(sizeof(uint64_t) * n, s), ds = dev_alloc(sizeof(int32_t) * n, s);
  Buf flags = dev_alloc(sizeof(BuildFlags), s);
  BuildFlags* hf = (BuildFlags*)pinned_scratch(sizeof(BuildFlags));
  *hf = BuildFlags{0ull, INT32_MAX, INT32_MAX, INT32_MAX, 0u};
  CS_HIP(hipMemcpyAsync(flags->p, hf, sizeof(BuildFlags), hipMemcpyHostToDevice, s));
  Buf values = dev_alloc(sizeof(int32_t) * n, s);
  hipLaunchKernelGGL(k_insert<T>, dim3(blocks_for(n)), dim3(kBlock), 0, s, items, nulls, n, ptr<unsigned long long>(table), slots - 1, ptr<uint64_t>(dk),
                     ptr<int32_t>(ds), ptr<BuildFlags>(flags), ptr<int32_t>(values));
  CS_HIP(hipGetLastError());
  CS_HIP(hipMemcpyAsync(hf, flags->p, sizeof(BuildFlags), hipMemcpyDeviceToHost, s));
  CS_HIP(hipStreamSynchronize(s));
  const BuildFlags f = *hf;
  int64_t k = (int64_t)f.distinct;
  if (f.saw_max) {
    hipLaunchKernelGGL(k_append_max, dim3(1), dim3(64), 0, s, ptr<uint64_t>(dk), ptr<int32_t>(ds), k);
    ++k;
  }
  radix_sort_pairs64(ptr<uint64_t>(dk), ptr<int32_t>(ds), k, s);
  const bool have_null = f.first_null != INT32_MAX;
  const int32_t base = have_null ? 1 : 0;
  auto c = blank(type, n, k + base, have_null, s);
  c->values = values;
  hipLaunchKernelGGL(k_rank<T>, dim3(blocks_for(std::max<int64_t>(k, 1))), dim3(kBlock), 0, s, ptr<const uint64_t>(dk), ptr<const int32_t>(ds), k, base, items,
                     have_null ? f.first_null : 0, f.first_zero == INT32_MAX ? -1 : f.first_zero, f.first_nan == INT32_MAX ? -1 : f.first_nan,
                     ptr<unsigned long long>(table), ptr<T>(c->keys));
  hipLaunchKernelGGL(k_values, dim3(blocks_for(n)), dim3(kBlock), 0, s, ptr<int32_t>(values), n, ptr<const unsigned long long>(table), base, (int32_t)(k - 1 + base));
  return finish(std::move(c), s);
}

// add / remove / set keys and merge.  `items` (n of them, `nulls` their bitmask) are the other key set; with `cat2` they
// are its keys and its values follow this category's.
template <class T>
cs_numcat* key_set_op(const cs_numcat* cat, int op, const T* items, int64_t n, const uint8_t* nulls, const cs_numcat* cat2, hipStream_t s) {
  const int32_t hn = cat->keys_have_null ? 1 : 0;
  const int64_t ko = cat->nkeys - hn;
  if (ko + n >= (1LL << 31) - 1) fail(CS_ERR_RANGE, "numeric category: more than 2^31 keys");
  const T* old_keys = ptr<const T>(cat->keys) + hn;
  // the items that are not null, in order
  Buf first_null = dev_alloc(sizeof(int32_t), s);
  hipLaunchKernelGGL(k_fill, dim3(1), dim3(kBlock), 0, s, ptr<int32_t>(first_null), (int64_t)1, INT32_MAX);
  Buf valid = dev_alloc(at_least(sizeof(int32_t) * n), s);
  if (n) hipLaunchKernelGGL(k_flag_valid, dim3(blocks_for(n)), dim3(kBlock), 0, s, nulls, n, ptr<int32_t>(valid), ptr<int32_t>(first_null));
  Compacted live = compact(ptr<const int32_t>(valid), n, s);
  const int32_t fnull = read_back<int32_t>(first_null->p, s);
  const bool new_null = cat2 ? cat2->keys_have_null : fnull != INT32_MAX;
  const int64_t m = live.n, all = ko + m;
  Buf img = dev_alloc(at_least(sizeof(uint64_t) * all), s), idx = dev_alloc(at_least(sizeof(int32_t) * all), s);
  if (ko) hipLaunchKernelGGL(k_images<T>, dim3(blocks_for(ko)), dim3(kBlock), 0, s, old_keys, (const int32_t*)nullptr, ko, (int64_t)0, 0, ptr<uint64_t>(img),
                             ptr<int32_t>(idx));
  if (m) hipLaunchKernelGGL(k_images<T>, dim3(blocks_for(m)), dim3(kBlock), 0, s, items, ptr<const int32_t>(live.pos), m, ko, (int32_t)ko, ptr<uint64_t>(img),
                            ptr<int32_t>(idx));
  radix_sort_pairs64(ptr<uint64_t>(img), ptr<int32_t>(idx), all, s);
  Buf heads = dev_alloc(at_least(sizeof(int32_t) * all), s);
  if (all) hipLaunchKernelGGL(k_heads, dim3(blocks_for(all)), dim3(kBlock), 0, s, ptr<const uint64_t>(img), ptr<const int32_t>(idx), all, (int32_t)ko, op,
                              ptr<int32_t>(heads));
  Compacted kept = compact(ptr<const int32_t>(heads), all, s);
  const bool have_null = op == OP_ADD ? (hn || new_null) : op == OP_REMOVE ? (hn && !new_null) : new_null;
  const int32_t base = have_null ? 1 : 0;
  const int64_t rows = cat->rows + (cat2 ? cat2->rows : 0);
  auto c = blank(cat->type, rows, kept.n + base, have_null, s);
  Buf table = dev_alloc(at_least(sizeof(int32_t) * cat->nkeys), s), table2;
  const int32_t hn2 = cat2 && cat2->keys_have_null ? 1 : 0;
  if (cat2) table2 = dev_alloc(at_least(sizeof(int32_t) * cat2->nkeys), s);
  if (hn) hipLaunchKernelGGL(k_fill, dim3(1), dim3(kBlock), 0, s, ptr<int32_t>(table), (int64_t)1, have_null ? 0 : -1);
  if (hn2) hipLaunchKernelGGL(k_fill, dim3(1), dim3(kBlock), 0, s, ptr<int32_t>(table2), (int64_t)1, 0);
  if (all) hipLaunchKernelGGL(k_emit<T>, dim3(blocks_for(all)), dim3(kBlock), 0, s, ptr<const int32_t>(idx), ptr<const int32_t>(heads), ptr<const int64_t>(kept.slot),
                              all, (int32_t)ko, old_keys, items, base, ptr<T>(c->keys), ptr<int32_t>(table) + hn, cat2 ? ptr<int32_t>(table2) + hn2 : nullptr);
  if (have_null) {  // the null key's number: this category's, else the lowest-indexed null item's (merge: the other category's)
    const T* from = hn ? ptr<const T>(cat->keys) : cat2 ? ptr<const T>(cat2->keys) : items + fnull;
    hipLaunchKernelGGL(k_copy_one<T>, dim3(1), dim3(64), 0, s, from, ptr<T>(c->keys));
  }
  if (cat->rows)
    hipLaunchKernelGGL(k_remap_values, dim3(blocks_for(cat->rows)), dim3(kBlock), 0, s, ptr<const int32_t>(cat->values), cat->rows, ptr<const int32_t>(table),
                       ptr<int32_t>(c->values));
  if (cat2 && cat2->rows)
    hipLaunchKernelGGL(k_remap_values, dim3(blocks_for(cat2->rows)), dim3(kBlock), 0, s, ptr<const int32_t>(cat2->values), cat2->rows,
                       ptr<const int32_t>(table2), ptr<int32_t>(c->values) + cat->rows);
  return finish(std::move(c), s);
}

cs_numcat* copy_cat(const cs_numcat* cat, hipStream_t s) {
  auto c = same_keys(cat, cat->rows, s);
  if (cat->rows) CS_HIP(hipMemcpyAsync(c->values->p, cat->values->p, sizeof(int32_t) * cat->rows, hipMemcpyDeviceToDevice, s));
  return finish(std::move(c), s);
}

// only the keys that `vals` (n of them, each in [lo_ok, nkeys) or the call fails) name; the values renumbered
cs_numcat* keep_used(const cs_numcat* cat, const int32_t* vals, int64_t n, int32_t lo_ok, const char* what, hipStream_t s) {
  const int64_t nk = cat->nkeys;
  Buf used = zeros32(nk, s), bad = zeros32(1, s);
  if (n) hipLaunchKernelGGL(k_mark_used, dim3(blocks_for(n)), dim3(kBlock), 0, s, vals, n, nk, lo_ok, ptr<int32_t>(used), ptr<unsigned>(bad));
  if (n && read_back<unsigned>(bad->p, s)) fail(CS_ERR_RANGE, std::string(what) + ": invalid index value");
  Compacted c = compact(ptr<const int32_t>(used), nk, s);
  const bool have_null = cat->keys_have_null && nk && read_back<int32_t>(used->p, s) != 0;
  auto res = blank(cat->type, n, c.n, have_null, s);
  Buf table = dev_alloc(at_least(sizeof(int32_t) * nk), s);
  if (nk) hipLaunchKernelGGL(k_table_from_slots, dim3(blocks_for(nk)), dim3(kBlock), 0, s, ptr<const int32_t>(used), ptr<const int64_t>(c.slot), nk, 0,
                             (const int32_t*)nullptr, ptr<int32_t>(table));
  if (c.n) dispatch(cat->type, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(k_gather_keys<T>, dim3(blocks_for(c.n)), dim3(kBlock), 0, s, ptr<const T>(cat->keys), ptr<const int32_t>(c.pos), c.n, ptr<T>(res->keys));
  });
  if (n) hipLaunchKernelGGL(k_remap_values, dim3(blocks_for(n)), dim3(kBlock), 0, s, vals, n, ptr<const int32_t>(table), ptr<int32_t>(res->values));
  return finish(std::move(res), s);
}

// index of `key` (host, one number of the category's type; NULL = the null key) among the keys, or -1
int32_t index_for(const cs_numcat* cat, const void* key, hipStream_t s) {
  const int32_t hn = cat->keys_have_null ? 1 : 0;
  if (!key) return hn ? 0 : -1;
  const int64_t ko = cat->nkeys - hn;
  if (ko == 0) return -1;
  Buf out = dev_alloc(sizeof(int32_t), s);
  hipLaunchKernelGGL(k_fill, dim3(1), dim3(kBlock), 0, s, ptr<int32_t>(out), (int64_t)1, -1);
  dispatch(cat->type, [&](auto t) {
    using T = decltype(t);
    T v;
    memcpy(&v, key, sizeof(T));
    hipLaunchKernelGGL(k_find<T>, dim3(blocks_for(ko)), dim3(kBlock), 0, s, ptr<const T>(cat->keys) + hn, ko, hn, Image<T>::of(v), ptr<int32_t>(out));
  });
  return read_back<int32_t>(out->p, s);
}

void check_positions(const int32_t* pos, int64_t n, int64_t limit, const char* what, hipStream_t s) {
  if (!n) return;
  Buf bad = zeros32(1, s);
  hipLaunchKernelGGL(k_check_range, dim3(blocks_for(n)), dim3(kBlock), 0, s, pos, n, limit, ptr<unsigned>(bad));
  if (read_back<unsigned>(bad->p, s)) fail(CS_ERR_RANGE, std::string(what) + ": invalid index value");
}
void write_mask(const int32_t* values, int64_t n, bool have_null, uint8_t* d_mask, hipStream_t s) {
  const int64_t nb = (n + 7) / 8;
  if (nb) hipLaunchKernelGGL(k_mask, dim3(blocks_for(nb)), dim3(kBlock), 0, s, values, n, have_null ? 1 : 0, d_mask, (unsigned long long*)nullptr);
}
void check_type(int type) {
  if (type < CS_NUM_I8 || type > CS_NUM_F64) fail(CS_ERR_INVALID_ARG, "numeric category: unknown type");
}
void check_rows(int64_t n) {
  if (n >= (1LL << 31) - 1) fail(CS_ERR_RANGE, "numeric category: more than 2^31 rows");
}

int key_set_entry(const char* what, int op, const cs_numcat* cat, const void* items, int64_t n, const uint8_t* nulls, int on_device, cs_stream stream,
                  cs_numcat** out) {
  return guard([&] {
    if (!cat || !out || n < 0) fail(CS_ERR_INVALID_ARG, std::string(what) + ": bad arguments");
    require_device();
    check_rows(n);
    hipStream_t s = S(stream);
    if (!items) n = 0;
    if (n == 0 && op != OP_SET) {  // .inl:490, 548: nothing to add or remove
      *out = copy_cat(cat, s);
      return;
    }
    dispatch(cat->type, [&](auto t) {
      using T = decltype(t);
      DevArray<T> in((const T*)items, n, on_device, s);
      DevArray<uint8_t> nl(n ? nulls : nullptr, (n + 7) / 8, on_device, s);
      *out = key_set_op<T>(cat, op, in.d, n, nl.d, nullptr, s);
    });
  });
}

}  // namespace

extern "C" {

int cs_numcat_build(const void* items, int64_t n, const uint8_t* nulls, cs_numtype type, int on_device, cs_stream stream, cs_numcat** out) {
  return guard([&] {
    if (!out || n < 0) fail(CS_ERR_INVALID_ARG, "numcat_build: bad arguments");
    check_type(type);
    require_device();
    check_rows(n);
    hipStream_t s = S(stream);
    dispatch(type, [&](auto t) {
      using T = decltype(t);
      DevArray<T> in((const T*)items, n, on_device, s);
      DevArray<uint8_t> nl(items ? nulls : nullptr, (n + 7) / 8, on_device, s);
      *out = build<T>(in.d, n, nl.d, s);
    });
  });
}
int cs_numcat_destroy(cs_numcat* cat) {
  return guard([&] { delete cat; });
}
int64_t cs_numcat_size(const cs_numcat* cat) { return cat ? cat->rows : 0; }
int64_t cs_numcat_keys_size(const cs_numcat* cat) { return cat ? cat->nkeys : 0; }
int cs_numcat_type(const cs_numcat* cat) { return cat ? cat->type : -1; }
const void* cs_numcat_keys_ptr(const cs_numcat* cat) { return cat && cat->nkeys ? cat->keys->p : nullptr; }
const int32_t* cs_numcat_values_ptr(const cs_numcat* cat) { return cat && cat->rows ? ptr<const int32_t>(cat->values) : nullptr; }
const uint8_t* cs_numcat_nulls_ptr(const cs_numcat* cat) { return cat ? ptr<const uint8_t>(cat->nulls) : nullptr; }
int cs_numcat_has_nulls(const cs_numcat* cat) { return cat && cat->null_rows > 0; }
int cs_numcat_keys_have_null(const cs_numcat* cat) { return cat && cat->keys_have_null; }

int cs_numcat_get_keys(const cs_numcat* cat, void* out, int on_device, cs_stream stream) {
  return guard([&] {
    if (!cat || (!out && cat->nkeys)) fail(CS_ERR_INVALID_ARG, "numcat_get_keys: bad arguments");
    require_device();
    const size_t bytes = (size_t)cat->nkeys * csnum::type_bytes(cat->type);
    if (bytes) CS_HIP(hipMemcpyAsync(out, cat->keys->p, bytes, on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, S(stream)));
    CS_HIP(hipStreamSynchronize(S(stream)));
  });
}
int cs_numcat_get_values(const cs_numcat* cat, int32_t* out, int on_device, cs_stream stream) {
  return guard([&] {
    if (!cat || (!out && cat->rows)) fail(CS_ERR_INVALID_ARG, "numcat_get_values: bad arguments");
    require_device();
    if (cat->rows) CS_HIP(hipMemcpyAsync(out, cat->values->p, sizeof(int32_t) * cat->rows, on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, S(stream)));
    CS_HIP(hipStreamSynchronize(S(stream)));
  });
}

int cs_numcat_to_type(const cs_numcat* cat, void* results, uint8_t* nulls, int on_device, cs_stream stream) {
  return guard([&] {
    if (!cat || (!results && cat->rows)) fail(CS_ERR_INVALID_ARG, "to_type: bad arguments");
    require_device();
    hipStream_t s = S(stream);
    const int64_t n = cat->rows;
    if (!n) return;
    ResultsOut res(results, (size_t)n * csnum::type_bytes(cat->type), on_device, s), mask(nulls, (size_t)((n + 7) / 8), on_device || !nulls, s);
    dispatch(cat->type, [&](auto t) {
      using T = decltype(t);
      hipLaunchKernelGGL(k_to_type<T>, dim3(blocks_for(n)), dim3(kBlock), 0, s, ptr<const T>(cat->keys), cat->nkeys, ptr<const int32_t>(cat->values), n, (T*)res.dev);
    });
    if (nulls) write_mask(ptr<const int32_t>(cat->values), n, cat->keys_have_null, (uint8_t*)mask.dev, s);
    CS_HIP(hipGetLastError());
    res.copy_back(s);
    if (nulls) mask.copy_back(s);
    CS_HIP(hipStreamSynchronize(s));
  });
}
int cs_numcat_gather_type(const cs_numcat* cat, const int32_t* indexes, int64_t n, void* results, uint8_t* nulls, int on_device, cs_stream stream) {
  return guard([&] {
    if (!cat || n < 0 || (n && (!indexes || !results))) fail(CS_ERR_INVALID_ARG, "gather_type: bad arguments");
    require_device();
    check_rows(n);
    hipStream_t s = S(stream);
    if (!n) return;
    DevArray<int32_t> p(indexes, n, on_device, s);
    check_positions(p.d, n, cat->nkeys, "gather_type", s);
    ResultsOut res(results, (size_t)n * csnum::type_bytes(cat->type), on_device, s), mask(nulls, (size_t)((n + 7) / 8), on_device || !nulls, s);
    dispatch(cat->type, [&](auto t) {
      using T = decltype(t);
      hipLaunchKernelGGL(k_to_type<T>, dim3(blocks_for(n)), dim3(kBlock), 0, s, ptr<const T>(cat->keys), cat->nkeys, p.d, n, (T*)res.dev);
    });
    if (nulls) write_mask(p.d, n, cat->keys_have_null, (uint8_t*)mask.dev, s);
    CS_HIP(hipGetLastError());
    res.copy_back(s);
    if (nulls) mask.copy_back(s);
    CS_HIP(hipStreamSynchronize(s));
  });
}
int cs_numcat_index_for(const cs_numcat* cat, const void* key, cs_stream stream, int32_t* out) {
  return guard([&] {
    if (!cat || !out) fail(CS_ERR_INVALID_ARG, "index_for: bad arguments");
    require_device();
    *out = index_for(cat, key, S(stream));
  });
}
int cs_numcat_indexes_for(const cs_numcat* cat, const void* key, int32_t* results, int on_device, cs_stream stream, int64_t* count) {
  return guard([&] {
    if (!cat || !count) fail(CS_ERR_INVALID_ARG, "indexes_for: bad arguments");
    require_device();
    hipStream_t s = S(stream);
    *count = 0;
    const int32_t k = index_for(cat, key, s);
    if (k < 0 || !cat->rows) return;
    if (!results) {  // the count alone: no compaction
      Buf cnt = zeroed_count(s);
      hipLaunchKernelGGL(k_count_equal, dim3(blocks_for(cat->rows)), dim3(kBlock), 0, s, ptr<const int32_t>(cat->values), cat->rows, k, ptr<unsigned long long>(cnt));
      *count = read_count(cnt, s);
      return;
    }
    Buf hit = dev_alloc(sizeof(int32_t) * cat->rows, s);
    hipLaunchKernelGGL(k_flag_equal, dim3(blocks_for(cat->rows)), dim3(kBlock), 0, s, ptr<const int32_t>(cat->values), cat->rows, k, ptr<int32_t>(hit));
    Compacted c = compact(ptr<const int32_t>(hit), cat->rows, s);
    *count = c.n;
    if (results && c.n)
      CS_HIP(hipMemcpyAsync(results, c.pos->p, sizeof(int32_t) * c.n, on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, s));
    CS_HIP(hipStreamSynchronize(s));
  });
}

int cs_numcat_add_keys(const cs_numcat* cat, const void* items, int64_t n, const uint8_t* nulls, int on_device, cs_stream stream, cs_numcat** out) {
  return key_set_entry("add_keys", OP_ADD, cat, items, n, nulls, on_device, stream, out);
}
int cs_numcat_remove_keys(const cs_numcat* cat, const void* items, int64_t n, const uint8_t* nulls, int on_device, cs_stream stream, cs_numcat** out) {
  return key_set_entry("remove_keys", OP_REMOVE, cat, items, n, nulls, on_device, stream, out);
}
int cs_numcat_set_keys(const cs_numcat* cat, const void* items, int64_t n, const uint8_t* nulls, int on_device, cs_stream stream, cs_numcat** out) {
  return key_set_entry("set_keys", OP_SET, cat, items, n, nulls, on_device, stream, out);
}
int cs_numcat_remove_unused_keys(const cs_numcat* cat, cs_stream stream, cs_numcat** out) {
  return guard([&] {
    if (!cat || !out) fail(CS_ERR_INVALID_ARG, "remove_unused_keys: bad arguments");
    require_device();
    *out = keep_used(cat, ptr<const int32_t>(cat->values), cat->rows, INT32_MIN, "remove_unused_keys", S(stream));
  });
}
int cs_numcat_merge(const cs_numcat* cat, const cs_numcat* cat2, cs_stream stream, cs_numcat** out) {
  return guard([&] {
    if (!cat || !cat2 || !out) fail(CS_ERR_INVALID_ARG, "merge: bad arguments");
    if (cat->type != cat2->type) fail(CS_ERR_INVALID_ARG, "merge: the categories hold different types");
    require_device();
    check_rows(cat->rows + cat2->rows);
    dispatch(cat->type, [&](auto t) {
      using T = decltype(t);
      const int hn2 = cat2->keys_have_null ? 1 : 0;
      *out = key_set_op<T>(cat, OP_ADD, ptr<const T>(cat2->keys) + hn2, cat2->nkeys - hn2, nullptr, cat2, S(stream));
    });
  });
}
int cs_numcat_gather(const cs_numcat* cat, const int32_t* indexes, int64_t n, int on_device, cs_stream stream, cs_numcat** out) {
  return guard([&] {
    if (!cat || !out || n < 0 || (n && !indexes)) fail(CS_ERR_INVALID_ARG, "gather: bad arguments");
    require_device();
    check_rows(n);
    hipStream_t s = S(stream);
    DevArray<int32_t> p(indexes, n, on_device, s);
    check_positions(p.d, n, cat->nkeys, "gather", s);
    auto c = same_keys(cat, n, s);
    if (n) CS_HIP(hipMemcpyAsync(c->values->p, p.d, sizeof(int32_t) * n, hipMemcpyDeviceToDevice, s));
    *out = finish(std::move(c), s);
  });
}
int cs_numcat_gather_and_remap(const cs_numcat* cat, const int32_t* indexes, int64_t n, int on_device, cs_stream stream, cs_numcat** out) {
  return guard([&] {
    if (!cat || !out || n < 0 || (n && !indexes)) fail(CS_ERR_INVALID_ARG, "gather_and_remap: bad arguments");
    require_device();
    check_rows(n);
    hipStream_t s = S(stream);
    DevArray<int32_t> p(indexes, n, on_device, s);
    *out = keep_used(cat, p.d, n, 0, "gather_and_remap", s);
  });
}
int cs_numcat_gather_values(const cs_numcat* cat, const int32_t* indexes, int64_t n, int on_device, cs_stream stream, cs_numcat** out) {
  return guard([&] {
    if (!cat || !out || n < 0 || (n && !indexes)) fail(CS_ERR_INVALID_ARG, "gather_values: bad arguments");
    require_device();
    check_rows(n);
    hipStream_t s = S(stream);
    DevArray<int32_t> p(indexes, n, on_device, s);
    auto c = same_keys(cat, n, s);
    if (n) {
      Buf bad = zeros32(1, s);
      hipLaunchKernelGGL(k_gather_values, dim3(blocks_for(n)), dim3(kBlock), 0, s, ptr<const int32_t>(cat->values), cat->rows, p.d, n, ptr<int32_t>(c->values),
                         ptr<unsigned>(bad));
      if (read_back<unsigned>(bad->p, s)) fail(CS_ERR_RANGE, "gather_values: invalid index value");
    }
    *out = finish(std::move(c), s);
  });
}
int cs_debug_numcat_sort_rows(const void* items, int64_t n, cs_numtype type, int on_device, cs_stream stream) {
  return guard([&] {
    if (!items || n <= 0) fail(CS_ERR_INVALID_ARG, "sort_rows: bad arguments");
    check_type(type);
    require_device();
    check_rows(n);
    hipStream_t s = S(stream);
    dispatch(type, [&](auto t) {
      using T = decltype(t);
      DevArray<T> in((const T*)items, n, on_device, s);
      Buf img = dev_alloc(sizeof(uint64_t) * n, s), idx = dev_alloc(sizeof(int32_t) * n, s);
      hipLaunchKernelGGL(k_images<T>, dim3(blocks_for(n)), dim3(kBlock), 0, s, in.d, (const int32_t*)nullptr, n, (int64_t)0, 0, ptr<uint64_t>(img), ptr<int32_t>(idx));
      radix_sort_pairs64(ptr<uint64_t>(img), ptr<int32_t>(idx), n, s);  // (waits for `s`: the buffers are idle when dropped)
      CS_HIP(hipGetLastError());
      CS_HIP(hipStreamSynchronize(s));
    });
  });
}
int cs_numcat_copy(const cs_numcat* cat, cs_stream stream, cs_numcat** out) {
  return guard([&] {
    if (!cat || !out) fail(CS_ERR_INVALID_ARG, "copy: bad arguments");
    require_device();
    *out = copy_cat(cat, S(stream));
  });
}

}  // extern "C"
