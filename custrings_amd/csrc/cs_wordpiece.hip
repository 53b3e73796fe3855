// WordPiece tokenization: a strings column to the int32 ids of a vocabulary.  The definition and the per-word logic are
// wordpiece_ops.h, shared with the CPU harness of tests/wordpiece_model.py.
//
// The vocabulary is built once into a hash table in device memory (a thread per vocabulary row inserts its one or two keys;
// an equal key keeps the lowest row by atomicMin) and handed out as a handle.  A row's ids come from one of two forms,
// chosen by the host as cs_minhash chooses:
//  - tile ("wordpiece tile"): short rows, the staged-row route.  A wave stages R = 64 / 32 / 16 rows in LDS and a lane walks
//    the words of its row out of LDS.
//  - long ("wordpiece long"): rows of any length, a wave per row, the bytes read from memory.  The row is cut into segments
//    of 64 bytes; the lanes whose byte starts a word take that word to its end -- also beyond the segment's -- and count its
//    ids, a wave scan places them behind the ids of the segments before, and the lanes match once more to put them.
// Each form serves three launches through one kernel template, the output an op struct (as sized_route.h has them): the ids
// per row (count), the ids at given offsets (write), and rows of max_length ids with specials, padding and mask (encode).
// No kernel waits for another workgroup, and nothing falls back to the host.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cstring>

#include "cs_internal.h"
#include "device_utils.h"
#include "tile_utils.h"
#include "wordpiece_ops.h"

using namespace cs;
using namespace csdev;

struct cs_wordpiece_vocab {
  Buf slots, chars;  // the table, and the vocabulary's chars its keys lie in
  cswp::Table table{};
  int64_t entries = 0;
  int max_entry_bytes = 0;
};

namespace {

// ---- the vocabulary ------------------------------------------------------------------------------------------------------------
struct DeviceAtomics {
  static __device__ __forceinline__ uint32_t cas(uint32_t* p, uint32_t expect, uint32_t v) { return atomicCAS(p, expect, v); }
  static __device__ __forceinline__ void lower(uint32_t* p, uint32_t v) { atomicMin(p, v); }
};
enum Info { I_ENTRIES = 0, I_MAX_WHOLE, I_MAX_CONT, I_FULL, kInfo };

__global__ void __launch_bounds__(256) k_wp_clear(cswp::Slot* __restrict__ slots, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) slots[i] = cswp::Slot{0u, cswp::kNoId, 0u, 0u};
}
__global__ void __launch_bounds__(256) k_wp_insert(ColView vocab, cswp::Prefix px, cswp::Slot* slots, uint32_t mask, uint32_t* __restrict__ info) {
  for (int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x; r < vocab.rows; r += (int64_t)gridDim.x * kBlock) {
    const bool valid = row_is_valid(vocab.validity, r);
    const int res = cswp::insert_row<DeviceAtomics>(slots, mask, vocab.chars, vocab.offsets, px, (int32_t)r, valid);
    if (res < 0) atomicOr(info + I_FULL, 1u);
    if (res > 0) atomicAdd(info + I_ENTRIES, 1u);
    const int len = valid ? (int)(vocab.offsets[r + 1] - vocab.offsets[r]) : 0;
    if (len <= 0 || len > cswp::kMaxEntryBytes) continue;
    atomicMax(info + I_MAX_WHOLE, (uint32_t)len);
    if (len > px.n && cswp::bytes_equal(vocab.chars + vocab.offsets[r], px.b, px.n)) atomicMax(info + I_MAX_CONT, (uint32_t)(len - px.n));
  }
}
// the id of one entry (create: unk; cs_wordpiece_vocab_find), by one thread
__global__ void k_wp_find(cswp::Table t, const uint8_t* __restrict__ text, int len, int32_t* __restrict__ id) {
  if (blockIdx.x == 0 && threadIdx.x == 0) *id = cswp::find_entry(t, text, len);
}

int32_t find_on_device(const cswp::Table& t, const char* text, size_t len, hipStream_t s) {
  if (len == 0 || len > (size_t)cswp::kMaxEntryBytes) return -1;
  const Buf d = dev_alloc(len + sizeof(int32_t) + 8, s);
  int32_t* id = ptr<int32_t>(d);
  uint8_t* bytes = ptr<uint8_t>(d) + 8;
  CS_HIP(hipMemcpyAsync(bytes, text, len, hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(k_wp_find, dim3(1), dim3(64), 0, s, t, bytes, (int)len, id);
  CS_HIP(hipGetLastError());
  return read_back<int32_t>(id, s);
}

// the table of `vocab` under `prefix`; the handle is complete but for table.unk
std::unique_ptr<cs_wordpiece_vocab> build_table(const cs_column* vocab, const cswp::Prefix& px, hipStream_t s) {
  auto v = std::make_unique<cs_wordpiece_vocab>();
  const int64_t nslots = cswp::slots_for(vocab->rows);
  v->slots = dev_alloc(sizeof(cswp::Slot) * (size_t)nslots, s);
  const Buf info = dev_alloc(sizeof(uint32_t) * kInfo, s);
  CS_HIP(hipMemsetAsync(info->p, 0, sizeof(uint32_t) * kInfo, s));
  hipLaunchKernelGGL(k_wp_clear, dim3(std::min(blocks_for(nslots), 65536u)), dim3(kBlock), 0, s, ptr<cswp::Slot>(v->slots), nslots);
  CS_HIP(hipGetLastError());
  if (vocab->rows > 0) {
    hipLaunchKernelGGL(k_wp_insert, dim3(std::min(blocks_for(vocab->rows), 65536u)), dim3(kBlock), 0, s, view_of(vocab), px, ptr<cswp::Slot>(v->slots),
                       (uint32_t)(nslots - 1), ptr<uint32_t>(info));
    CS_HIP(hipGetLastError());
  }
  uint32_t* h = (uint32_t*)pinned_scratch(sizeof(uint32_t) * kInfo);
  CS_HIP(hipMemcpyAsync(h, info->p, sizeof(uint32_t) * kInfo, hipMemcpyDeviceToHost, s));
  CS_HIP(hipStreamSynchronize(s));
  if (h[I_FULL]) fail(CS_ERR_INTERNAL, "wordpiece: the vocabulary's table ran full");
  v->entries = h[I_ENTRIES];
  v->max_entry_bytes = (int)h[I_MAX_WHOLE];
  v->chars = dev_owned(vocab->chars, s);  // (the keys' bytes outlive a borrowed column)
  v->table = cswp::Table{ptr<const cswp::Slot>(v->slots), ptr<const uint8_t>(v->chars), (uint32_t)(nslots - 1), {(int)h[I_MAX_WHOLE], (int)h[I_MAX_CONT]}, -1};
  return v;
}

// ---- the outputs of a launch ---------------------------------------------------------------------------------------------------
// An output names: kPuts (false: the ids themselves are not wanted), limit() (the ids of a row it takes at most), put(r)
// (the functor (k, id) for id k of row r) and finish(r, count, j0, step), called once the row's `count` ids are put, by its
// one lane (j0 = 0, step = 1) or by every lane of its wave (j0 = lane, step = 64): the positions j0, j0 + step, ... are the
// caller's to fill.
struct PutWithin {  // id k of a row at at[k], for k < n
  int32_t* at;
  int n;
  __device__ __forceinline__ void operator()(int k, int32_t id) const {
    if (k < n) at[k] = id;
  }
};
struct CountOut {
  int32_t* lens;
  static constexpr bool kPuts = false;
  __device__ __forceinline__ int limit() const { return INT_MAX; }
  __device__ __forceinline__ cswp::NoOutput put(int64_t) const { return cswp::NoOutput{}; }
  __device__ __forceinline__ void finish(int64_t r, int count, int j0, int) const {
    if (j0 == 0) lens[r] = count;
  }
};
struct WriteOut {  // (a row never writes beyond its own offsets, whatever they are)
  const int64_t* off;
  int32_t* ids;
  static constexpr bool kPuts = true;
  __device__ __forceinline__ int limit() const { return INT_MAX; }
  __device__ __forceinline__ PutWithin put(int64_t r) const {
    const int64_t o = off[r], n = off[r + 1] - o;
    return PutWithin{ids + o, (int)(n < 0 ? 0 : n > INT_MAX ? INT_MAX : n)};
  }
  __device__ __forceinline__ void finish(int64_t, int, int, int) const {}
};
struct EncodeOut {
  cswp::Specials sp;
  int32_t* ids;
  uint8_t* mask;  // may be null
  static constexpr bool kPuts = true;
  __device__ __forceinline__ int limit() const { return sp.room(); }
  __device__ __forceinline__ PutWithin put(int64_t r) const { return PutWithin{ids + r * sp.max_length + sp.front(), sp.room()}; }
  __device__ __forceinline__ void finish(int64_t r, int count, int j0, int step) const {
    const int kept = min(count, sp.room()), first = sp.front(), used = cswp::used(sp, kept);
    int32_t* row = ids + r * sp.max_length;
    for (int j = j0; j < sp.max_length; j += step) {
      if (j < first || j >= first + kept) row[j] = cswp::filler(sp, kept, j);
      if (mask) mask[r * sp.max_length + j] = j < used;
    }
  }
};

struct WpArgs {
  ColView in;
  cswp::Table t;
  int max_word_chars, punct;
  int rows_per_tile, cap;  // tile form
  long long ntiles;
};

template <class Out>
__global__ void __launch_bounds__(256) k_wordpiece_tile(WpArgs a, Out out) {
  extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
  uint8_t* lds_in = reinterpret_cast<uint8_t*>(smem) + (size_t)wv * a.cap;
  // (every tile's span fits the staging buffer: checked by the host)
  cstile::walk_staged_tiles<cstile::Oversize::kHostChecked>(a.in, a.rows_per_tile, a.ntiles, lds_in, a.cap, wv, lane,
                                                            [&](const cstile::RowTile& cur, const uint8_t* p) {
    if (!cur.in_tile) return;
    const int64_t r = cur.r0 + lane;
    const int count = cswp::row_ids(a.t, p, cur.n, a.max_word_chars, a.punct, out.limit(), out.put(r));
    out.finish(r, count, 0, 1);
  });
}

template <class Out>
__global__ void __launch_bounds__(256) k_wordpiece_long(WpArgs a, Out out) {
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
  for (int64_t r = (int64_t)blockIdx.x * 4 + wv; r < a.in.rows; r += (int64_t)gridDim.x * 4) {
    const int64_t o0 = a.in.offsets[r];
    const int n = row_is_valid(a.in.validity, r) ? (int)(a.in.offsets[r + 1] - o0) : 0;
    const uint8_t* p = a.in.chars + o0;
    const auto put = out.put(r);
    const int limit = out.limit();
    int base = 0;  // the ids of the segments before
    for (int seg = 0; seg < n && base < limit; seg += 64) {
      const int pos = seg + lane;
      const bool mine = pos < n && cswp::word_starts_at(p, pos, a.punct);
      if (!__ballot(mine)) continue;
      int hi = pos, nch = 0, cnt = 0;
      if (mine) {
        hi = cswp::word_end(p, n, pos, a.punct, nch);
        cnt = cswp::match_word(a.t, p + pos, hi - pos, nch, a.max_word_chars, 0, cswp::NoOutput{});
      }
      const int incl = wave_inclusive_scan(cnt);
      if (Out::kPuts && mine) {
        // (only the word's own places: a word that fails half way must not reach into the next lane's)
        const int k0 = base + incl - cnt, k1 = base + incl;
        cswp::match_word(a.t, p + pos, hi - pos, nch, a.max_word_chars, k0, [&](int k, int32_t id) {
          if (k < k1) put(k, id);
        });
      }
      base += __builtin_amdgcn_readlane(incl, 63);
    }
    out.finish(r, base, lane, 64);
  }
}

// one tokenizing call, all of its parameters in sight
struct WpCall {
  const cs_column* col;
  const cs_wordpiece_vocab* v;
  int max_word_chars, punct;
  hipStream_t s;
};

bool long_form_only() { return cfg_int("CS_WORDPIECE_LONG", 0) != 0; }

template <class Out>
void run_wordpiece(const WpCall& c, const Out& out) {
  WpArgs a{};
  a.in = view_of(c.col);
  a.t = c.v->table;
  a.max_word_chars = c.max_word_chars;
  a.punct = c.punct != 0;
  StagedTiles t;
  if (!long_form_only()) t = plan_staged_tiles(c.col, cstile::kStageSlack, false, {1, 0, 150 * 1024}, c.s);
  ProfScope ps("k_wordpiece", c.s);
  if (t.R) {
    a.rows_per_tile = t.R;
    a.cap = t.cap;
    a.ntiles = t.ntiles;
    launch_resident(&k_wordpiece_tile<Out>, t.lds, t.grid, c.s, a, out);
    note_route("wordpiece tile");
  } else {
    launch_resident(&k_wordpiece_long<Out>, 0, (c.col->rows + 3) / 4, c.s, a, out);
    note_route("wordpiece long");
  }
}

WpCall checked_call(const cs_column* col, const cs_wordpiece_vocab* v, int max_word_chars, int punct, cs_stream stream) {
  if (!col || !v) fail(CS_ERR_INVALID_ARG, "wordpiece: null column or vocabulary");
  if (max_word_chars < 1 || max_word_chars > cswp::kMaxWordChars) fail(CS_ERR_RANGE, "wordpiece: max_word_chars is 1 to 1024");
  return WpCall{col, v, max_word_chars, punct, S(stream)};
}

}  // namespace

extern "C" {

int cs_wordpiece_vocab_create(const cs_column* vocab, const char* prefix, const char* unk, cs_stream stream, cs_wordpiece_vocab** out) {
  return guard([&] {
    if (!vocab || !out) fail(CS_ERR_INVALID_ARG, "wordpiece: null vocabulary or output");
    *out = nullptr;
    if (!prefix) prefix = "##";
    if (!unk) unk = "[UNK]";
    cswp::Prefix px{};
    const size_t plen = strlen(prefix);
    if (plen < 1 || plen > (size_t)cswp::kMaxPrefix) fail(CS_ERR_INVALID_ARG, "wordpiece: the prefix has 1 to 8 bytes");
    memcpy(px.b, prefix, plen);
    px.n = (int)plen;
    if (vocab->rows > cswp::kMaxEntries) fail(CS_ERR_RANGE, "wordpiece: a vocabulary has at most 2^24 rows");
    require_device();
    const hipStream_t s = S(stream);
    if (vocab->rows > 0 && max_row_bytes(vocab, s) > cswp::kMaxEntryBytes) fail(CS_ERR_RANGE, "wordpiece: an entry has at most 255 bytes");
    std::unique_ptr<cs_wordpiece_vocab> v = build_table(vocab, px, s);
    v->table.unk = find_on_device(v->table, unk, strlen(unk), s);
    if (v->table.unk < 0) fail(CS_ERR_INVALID_ARG, "wordpiece: the unknown token is no entry of the vocabulary");
    *out = v.release();
  });
}

void cs_wordpiece_vocab_destroy(cs_wordpiece_vocab* v) { delete v; }

int cs_wordpiece_vocab_info(const cs_wordpiece_vocab* v, int64_t* entries, int32_t* unk_id, int32_t* max_entry_bytes) {
  return guard([&] {
    if (!v) fail(CS_ERR_INVALID_ARG, "wordpiece: null vocabulary");
    if (entries) *entries = v->entries;
    if (unk_id) *unk_id = v->table.unk;
    if (max_entry_bytes) *max_entry_bytes = v->max_entry_bytes;
  });
}

int cs_wordpiece_vocab_find(const cs_wordpiece_vocab* v, const char* token, int64_t nbytes, int32_t* id, cs_stream stream) {
  return guard([&] {
    if (!v || !id || (!token && nbytes != 0) || nbytes < 0) fail(CS_ERR_INVALID_ARG, "wordpiece: bad arguments");
    require_device();
    *id = find_on_device(v->table, token, (size_t)nbytes, S(stream));
  });
}

int cs_wordpiece_count(const cs_column* col, const cs_wordpiece_vocab* v, int max_word_chars, int punct, int64_t* offsets, int on_device, cs_stream stream,
                       int64_t* total) {
  return guard([&] {
    const WpCall c = checked_call(col, v, max_word_chars, punct, stream);
    if (!offsets || !total) fail(CS_ERR_INVALID_ARG, "wordpiece: null offsets or total");
    *total = 0;
    require_device();
    const int64_t rows = col->rows;
    const ResultsOut res(offsets, sizeof(int64_t) * (size_t)(rows + 1), on_device, c.s);
    if (rows == 0) {
      CS_HIP(hipMemsetAsync(res.dev, 0, sizeof(int64_t), c.s));
    } else {
      const Buf lens = dev_alloc(sizeof(int32_t) * (size_t)rows, c.s);
      run_wordpiece(c, CountOut{ptr<int32_t>(lens)});
      offsets_from_lengths_async(ptr<const int32_t>(lens), rows, static_cast<int64_t*>(res.dev), c.s);
      *total = read_back<int64_t>(static_cast<const int64_t*>(res.dev) + rows, c.s);  // (`lens` goes back to the pool behind this)
    }
    res.finish(c.s);
  });
}

int cs_wordpiece_ids(const cs_column* col, const cs_wordpiece_vocab* v, int max_word_chars, int punct, const int64_t* offsets, int32_t* ids, int on_device,
                     cs_stream stream) {
  return guard([&] {
    const WpCall c = checked_call(col, v, max_word_chars, punct, stream);
    if (!offsets) fail(CS_ERR_INVALID_ARG, "wordpiece: null offsets");
    const int64_t rows = col->rows;
    if (!ids || rows == 0) return;  // nothing is written
    require_device();
    const DevArray<int64_t> off(offsets, rows + 1, on_device, c.s);
    const int64_t first = on_device ? read_back<int64_t>(off.d, c.s) : offsets[0];
    const int64_t total = on_device ? read_back<int64_t>(off.d + rows, c.s) : offsets[rows];
    if (first != 0 || total < 0) fail(CS_ERR_INVALID_ARG, "wordpiece: the offsets are not cs_wordpiece_count's");
    if (total == 0) return;
    const ResultsOut res(ids, sizeof(int32_t) * (size_t)total, on_device, c.s);
    run_wordpiece(c, WriteOut{off.d, static_cast<int32_t*>(res.dev)});
    res.finish(c.s);
  });
}

int cs_wordpiece_encode(const cs_column* col, const cs_wordpiece_vocab* v, int max_word_chars, int punct, int max_length, int32_t cls_id, int32_t sep_id,
                        int32_t pad_id, int32_t* ids, uint8_t* mask, int on_device, cs_stream stream) {
  return guard([&] {
    const WpCall c = checked_call(col, v, max_word_chars, punct, stream);
    const cswp::Specials sp{cls_id, sep_id, pad_id, max_length};
    if (max_length < 1 || sp.room() < 0) fail(CS_ERR_INVALID_ARG, "wordpiece: max_length is less than the special ids take");
    const int64_t rows = col->rows;
    if (!ids || rows == 0) return;  // nothing is written
    require_device();
    const size_t cells = (size_t)rows * (size_t)max_length;
    const ResultsOut rid(ids, sizeof(int32_t) * cells, on_device, c.s);
    const ResultsOut rmask(mask, mask ? cells : 0, mask ? on_device : 1, c.s);
    run_wordpiece(c, EncodeOut{sp, static_cast<int32_t*>(rid.dev), static_cast<uint8_t*>(rmask.dev)});
    rmask.copy_back(c.s);
    rid.finish(c.s);
  });
}

}  // extern "C"
