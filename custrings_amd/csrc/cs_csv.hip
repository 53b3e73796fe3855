// from_csv (reference: cpp/src/util.cu:42-169, createFromCSV): one column of a CSV text as a strings column.  The byte
// rules are csv_ops.h, shared with the CPU harness of tests/test_csv_cpu.py.
//
// The text is the caller's `n` bytes, then the '\r' the loader appends at position n and a NUL at n + 1; it ends at its first
// NUL, Z.  A host text is uploaded with the '\r' behind it; device bytes are read where they are, the two bytes behind them
// exist in the kernels' reading only.  Nothing is written into the text.
//
// Line starts (csv_ops.h: a three-state walk, a 16-byte piece per lane, one addition per piece), two levels:
//   k_csv_tile_summary  a workgroup per tile of kTileBytes: the tile as a function of the state it is entered in (a
//                       2-bit result for each of the three states), its count of line starts when entered in state 0, whether
//                       state 2 adds one (the first byte behind the tile's leading control bytes), and the first NUL
//   k_csv_tile_scan     one workgroup over the tile summaries: each tile's entry state and the count of starts before it
//   k_csv_write_starts  the tile pass again, now writing each start to its place (up to `lines` + 1 of them, none beyond Z)
// Inside a tile the lanes' entry states come from ballots (the nearest lower lane that is not all control bytes decides, the
// all-control lanes between add their terminators) and the waves' from a walk over the four wave functions in LDS.
//
// Fields: the rows are a column over the text whose offsets are the starts -- chars contiguous, no validity --, so the
// field walk is a parser of parse_route.h (tile route, and rows where a span exceeds a staged tile; CS_CSV_ROWWISE=1) whose
// result is csv_ops.h's (begin, length).  k_csv_spans turns them into (pointer, length) pairs and the span copy behind
// create_from_index builds the column (the sort if asked, LenMeta handed on).  With device bytes the last row may hold the
// appended '\r': that row alone is parsed and copied from a copy of its span with the '\r' behind it.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

#include "cs_internal.h"
#include "csv_ops.h"
#include "device_utils.h"
#include "parse_route.h"

using namespace cs;
using namespace csdev;
using cscsv::Field;
using cscsv::Piece;

namespace {

constexpr int kTileBytes = kBlock * cscsv::kPieceBytes;
constexpr int kWaves = kBlock / kWave;
constexpr uint32_t kIdentity = 0 | (1 << 2) | (2 << 4);  // a state function as a table: two bits for each state it is entered in

__device__ __forceinline__ int apply(uint32_t table, int state) { return (table >> (2 * state)) & 3; }

struct Text {
  const uint8_t* bytes;
  int64_t n;  // real bytes; position n reads '\r', every position behind it 0
};
__device__ __forceinline__ uint8_t text_byte(const Text& t, int64_t p) { return p < t.n ? t.bytes[p] : (p == t.n ? (uint8_t)'\r' : (uint8_t)0); }

// the piece of this lane: 16 bytes at p (a multiple of 16)
__device__ __forceinline__ Piece load_piece(const Text& t, int64_t p) {
  uint32_t w[4];
  if (p + cscsv::kPieceBytes <= t.n && (reinterpret_cast<uintptr_t>(t.bytes) & 15) == 0) {
    const uint4 q = *reinterpret_cast<const uint4*>(t.bytes + p);
    w[0] = q.x, w[1] = q.y, w[2] = q.z, w[3] = q.w;
  } else {
    for (int k = 0; k < 4; ++k) {
      w[k] = 0;
      for (int j = 0; j < 4; ++j) w[k] |= (uint32_t)text_byte(t, p + 4 * k + j) << (8 * j);
    }
  }
  return cscsv::classify(w);
}

// What a tile pass knows of its lanes: each lane's piece and, for the state the WAVE is entered in, the lane's entry state.
struct WaveWalk {
  unsigned long long decides, ends2, ends1, adds;  // ballots: lanes that are not all control bytes; their end state 2 / >= 1;
                                                   // all-control lanes that hold a terminator
  // the state in front of `lane` (64: behind the wave) when the wave is entered in `in`
  __device__ __forceinline__ int state_before(int lane, int in) const {
    const unsigned long long lower = lane >= 64 ? ~0ull : (1ull << lane) - 1;
    const unsigned long long below = decides & lower;
    int base = in;
    unsigned long long between = lower;
    if (below) {
      const int j = 63 - __builtin_clzll(below);
      base = ((ends2 >> j) & 1) ? 2 : (int)((ends1 >> j) & 1);
      between = lower & ~((2ull << j) - 1);  // (j = 63: the shift wraps to 0 and nothing is between)
    }
    if (adds & between) return 2;
    return between ? max(base, 1) : base;
  }
};
__device__ __forceinline__ WaveWalk walk_wave(const Piece& pc) {
  const bool all_control = pc.control == 0xFFFFu;
  int end;
  cscsv::piece_starts(pc, 0, end);
  WaveWalk w;
  w.decides = __ballot(!all_control);
  w.ends2 = __ballot(!all_control && end == 2);
  w.ends1 = __ballot(!all_control && end >= 1);
  w.adds = __ballot(all_control && pc.terminator != 0);
  return w;
}

// The tile of this workgroup: every thread gets its piece, its wave's walk and the four wave functions (tables).
struct TileWalk {
  Piece pc;
  WaveWalk wave;
  uint32_t wave_table[kWaves];
  int first_nul;  // position in the tile of its first NUL, kTileBytes when it has none
  __device__ __forceinline__ int wave_entry(int wv, int tile_in) const {
    int s = tile_in;
    for (int k = 0; k < wv; ++k) s = apply(wave_table[k], s);
    return s;
  }
  __device__ __forceinline__ uint32_t tile_table() const {
    uint32_t t = 0;
    for (int in = 0; in < 3; ++in) t |= (uint32_t)wave_entry(kWaves, in) << (2 * in);
    return t;
  }
  // this lane's line starts (a mask over its piece) when the tile is entered in `tile_in`; none behind `last` (tile position)
  __device__ __forceinline__ uint32_t starts(int tile_in, int last) const {
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    int out;
    const uint32_t m = cscsv::piece_starts(pc, wave.state_before(lane, wave_entry(wv, tile_in)), out);
    const int room = last - (int)threadIdx.x * cscsv::kPieceBytes + 1;  // bytes of the piece at or before `last`
    return room <= 0 ? 0u : (room >= cscsv::kPieceBytes ? m : m & ((1u << room) - 1));
  }
};
__device__ __forceinline__ TileWalk walk_tile(const Text& t, int64_t tile) {
  __shared__ uint32_t s_table[kWaves];
  __shared__ int s_nul[kWaves];
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  TileWalk w;
  w.pc = load_piece(t, tile * kTileBytes + (int64_t)threadIdx.x * cscsv::kPieceBytes);
  w.wave = walk_wave(w.pc);
  int nul = w.pc.nul ? (int)threadIdx.x * cscsv::kPieceBytes + __builtin_ctz(w.pc.nul) : kTileBytes;
  for (int d = kWave / 2; d > 0; d >>= 1) nul = min(nul, __shfl_xor(nul, d, kWave));
  if (lane == 0) {
    uint32_t tab = 0;
    for (int in = 0; in < 3; ++in) tab |= (uint32_t)w.wave.state_before(64, in) << (2 * in);
    s_table[wv] = tab;
    s_nul[wv] = nul;
  }
  __syncthreads();
  w.first_nul = kTileBytes;
  for (int k = 0; k < kWaves; ++k) {
    w.wave_table[k] = s_table[k];
    w.first_nul = min(w.first_nul, s_nul[k]);
  }
  return w;
}

// a tile's summary word: its table (6 bits), its starts when entered in state 0 or 1 (<= kTileBytes: 13 bits), one more in state 2
constexpr int kCountShift = 6, kExtraShift = 20;
constexpr uint32_t kCountMask = 0x1FFF;

// heads[0]: the first NUL of the text (atomicMin; ~0 before), heads[1]: the count of line starts (k_csv_tile_scan)
__global__ void __launch_bounds__(kBlock) k_csv_tile_summary(Text t, uint32_t* __restrict__ summary, unsigned long long* __restrict__ heads) {
  const int64_t tile = blockIdx.x;
  const TileWalk w = walk_tile(t, tile);
  // (a NUL is no control byte: the first byte behind the leading control bytes is at or before it)
  const int c0 = __popc(w.starts(0, w.first_nul)), c2 = __popc(w.starts(2, w.first_nul));
  const long long both = block_reduce_sum(c0 | (c2 << 16));
  if (threadIdx.x == 0) {
    const uint32_t n0 = (uint32_t)both & 0xFFFFu, n2 = (uint32_t)(both >> 16) & 0xFFFFu;
    summary[tile] = w.tile_table() | (n0 << kCountShift) | ((n2 - n0) << kExtraShift);
    if (w.first_nul < kTileBytes) atomicMin(heads, (unsigned long long)(tile * kTileBytes + w.first_nul));
  }
}

// One workgroup: thread j takes the tiles [j * per, (j + 1) * per).  Three walks over them: the chunk as a function, the
// tiles' entry states and counts once thread 0 has chained the chunks, the chunks' bases added.
__global__ void __launch_bounds__(kBlock) k_csv_tile_scan(const uint32_t* __restrict__ summary, int64_t ntiles, unsigned long long* __restrict__ heads,
                                                           uint8_t* __restrict__ tile_in, int64_t* __restrict__ tile_first) {
  __shared__ uint32_t s_table[kBlock];
  __shared__ int s_in[kBlock];
  __shared__ long long s_count[kBlock];
  const int64_t per = (ntiles + kBlock - 1) / kBlock;
  const int64_t t0 = std::min<int64_t>(ntiles, (int64_t)threadIdx.x * per), t1 = std::min<int64_t>(ntiles, t0 + per);
  const int64_t last_tile = (int64_t)(heads[0] / kTileBytes);  // the tile of the first NUL: no start behind it
  uint32_t table = kIdentity;
  for (int64_t t = t0; t < t1; ++t) {
    const uint32_t next = summary[t];
    uint32_t both = 0;
    for (int in = 0; in < 3; ++in) both |= (uint32_t)apply(next, apply(table, in)) << (2 * in);
    table = both;
  }
  s_table[threadIdx.x] = table;
  __syncthreads();
  if (threadIdx.x == 0) {
    int s = 0;  // the text begins outside any run of control bytes
    for (int j = 0; j < kBlock; ++j) {
      s_in[j] = s;
      s = apply(s_table[j], s);
    }
  }
  __syncthreads();
  int s = s_in[threadIdx.x];
  long long count = 0;
  for (int64_t t = t0; t < t1; ++t) {
    const uint32_t word = summary[t];
    tile_in[t] = (uint8_t)s;
    tile_first[t] = count;
    if (t <= last_tile) count += ((word >> kCountShift) & kCountMask) + (s == 2 ? (word >> kExtraShift) & 1 : 0);
    s = apply(word, s);
  }
  s_count[threadIdx.x] = count;
  __syncthreads();
  if (threadIdx.x == 0) {
    long long before = 0;
    for (int j = 0; j < kBlock; ++j) {
      const long long c = s_count[j];
      s_count[j] = before;
      before += c;
    }
    heads[1] = (unsigned long long)before;
  }
  __syncthreads();
  const long long base = s_count[threadIdx.x];
  for (int64_t t = t0; t < t1; ++t) tile_first[t] += base;
}

__global__ void __launch_bounds__(kBlock) k_csv_write_starts(Text t, const unsigned long long* __restrict__ heads, const uint8_t* __restrict__ tile_in,
                                                              const int64_t* __restrict__ tile_first, int64_t limit, int64_t* __restrict__ starts) {
  const int64_t tile = blockIdx.x, p0 = tile * kTileBytes;
  const int64_t z = (int64_t)heads[0];
  if (p0 > z || tile_first[tile] >= limit) return;  // (the whole workgroup)
  const TileWalk w = walk_tile(t, tile);
  uint32_t m = w.starts(tile_in[tile], (int)std::min<int64_t>(z - p0, kTileBytes - 1));
  int64_t at = tile_first[tile] + block_exclusive_scan(__popc(m), nullptr);
  const int64_t p = p0 + (int64_t)threadIdx.x * cscsv::kPieceBytes;
  for (; m && at < limit; m &= m - 1, ++at) starts[at] = p + __builtin_ctz(m);
}

// ---- fields ------------------------------------------------------------------------------------------------------------------
struct FieldParser {
  using T = Field;
  static constexpr bool kCounted = false;
  unsigned column;
  bool null_is_empty;
  __device__ __forceinline__ Field operator()(const uint8_t* p, int n, bool) const { return cscsv::locate_field(p, n, column, null_is_empty); }
};
struct Span {  // std::pair<const char*, size_t>
  const char* p;
  size_t n;
};
// rows [0, rows) of the text; a row at or behind `tail_row` (the one row that holds the appended '\r') lies in `tail`
__global__ void __launch_bounds__(kBlock) k_csv_spans(const uint8_t* __restrict__ text, const int64_t* __restrict__ starts, const Field* __restrict__ fields,
                                                       int64_t rows, int64_t tail_row, const uint8_t* __restrict__ tail, Span* __restrict__ spans) {
  const int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (r >= rows) return;
  const Field f = fields[r];
  const uint8_t* row = r >= tail_row ? tail : text + starts[r];
  spans[r].p = f.is_null() ? nullptr : reinterpret_cast<const char*>(row + f.begin);
  spans[r].n = f.is_null() ? 0 : (size_t)f.length;
}

// a column over borrowed chars and offsets: `rows` rows from offsets[0]
void borrow_rows(cs_column& c, const uint8_t* chars, int64_t nbytes, const Buf& offsets, int64_t rows) {
  c.rows = rows;
  c.nbytes = nbytes;
  c.null_count = 0;
  c.chars = dev_wrap(chars, (size_t)nbytes);
  c.offsets = offsets;
}
void locate_fields(const cs_column& lines, const FieldParser& parser, Field* out, hipStream_t s) {
  if (lines.rows == 0) return;
  // (spans are clamped to 2^31 - 1 when they are measured)
  if (max_span64(&lines, s) >= 0x7fffffff && max_row_bytes(&lines, s) >= 0x7fffffff) fail(CS_ERR_RANGE, "from_csv: a row of 2^31 - 1 bytes or more");
  csparse::launch_parse(&lines, parser, out, nullptr, !cfg("CS_CSV_ROWWISE"), s);
}

// `bytes`: device memory; `cr_in_memory`: bytes[n] is readable and holds the appended '\r'
cs_column* csv_column(const uint8_t* bytes, int64_t n, bool cr_in_memory, unsigned column, unsigned lines, unsigned flags, hipStream_t s) {
  const Text text{bytes, n};
  const int64_t ntiles = (n + 2 + kTileBytes - 1) / kTileBytes;
  Buf summary = dev_alloc(sizeof(uint32_t) * (size_t)ntiles, s), tile_in = dev_alloc((size_t)ntiles, s);
  Buf tile_first = dev_alloc(sizeof(int64_t) * (size_t)ntiles, s), heads = dev_alloc(2 * sizeof(unsigned long long), s);
  CS_HIP(hipMemsetAsync(heads->p, 0xFF, sizeof(unsigned long long), s));
  unsigned long long* d_heads = ptr<unsigned long long>(heads);
  int64_t* host = (int64_t*)pinned_scratch(3 * sizeof(int64_t));
  {
    ProfScope prof("k_csv_line_starts", s);
    hipLaunchKernelGGL(k_csv_tile_summary, dim3((unsigned)ntiles), dim3(kBlock), 0, s, text, ptr<uint32_t>(summary), d_heads);
    hipLaunchKernelGGL(k_csv_tile_scan, dim3(1), dim3(kBlock), 0, s, ptr<const uint32_t>(summary), ntiles, d_heads, ptr<uint8_t>(tile_in), ptr<int64_t>(tile_first));
    CS_HIP(hipGetLastError());
  }
  CS_HIP(hipMemcpyAsync(host, heads->p, 2 * sizeof(int64_t), hipMemcpyDeviceToHost, s));
  CS_HIP(hipStreamSynchronize(s));
  const int64_t first_nul = host[0], found = host[1];
  const int64_t nstarts = lines ? std::min<int64_t>(found, (int64_t)lines + 1) : found;
  const int64_t rows = nstarts - 1;  // the header has no recorded start and yields no row
  if (rows <= 0) return make_all_null(0, s);
  Buf starts = dev_alloc(sizeof(int64_t) * (size_t)nstarts, s);
  {
    ProfScope prof("k_csv_line_starts", s);
    hipLaunchKernelGGL(k_csv_write_starts, dim3((unsigned)ntiles), dim3(kBlock), 0, s, text, d_heads, ptr<const uint8_t>(tile_in), ptr<const int64_t>(tile_first),
                       nstarts, ptr<int64_t>(starts));
    CS_HIP(hipGetLastError());
  }
  // With no NUL in the caller's bytes the last start is n + 1 and the last row holds the appended '\r' at n.
  const bool tail_row = !cr_in_memory && first_nul == n + 1 && nstarts == found;
  const int64_t in_place = tail_row ? rows - 1 : rows;
  Buf fields = dev_alloc(sizeof(Field) * (size_t)rows, s), tail;
  const FieldParser parser{column, (flags & cscsv::kNullIsEmpty) != 0};
  {
    ProfScope prof("k_csv_fields", s);
    if (tail_row) {
      CS_HIP(hipMemcpyAsync(host + 2, ptr<int64_t>(starts) + rows - 1, sizeof(int64_t), hipMemcpyDeviceToHost, s));
      CS_HIP(hipStreamSynchronize(s));
      const int64_t from = host[2], span = n + 1 - from;
      if (span >= 0x7fffffff) fail(CS_ERR_RANGE, "from_csv: a row of 2^31 - 1 bytes or more");
      tail = dev_alloc((size_t)span, s);
      if (span > 1) CS_HIP(hipMemcpyAsync(tail->p, bytes + from, (size_t)(span - 1), hipMemcpyDeviceToDevice, s));
      CS_HIP(hipMemsetAsync(ptr<uint8_t>(tail) + span - 1, '\r', 1, s));
      Buf ends = dev_alloc(2 * sizeof(int64_t), s);
      const int64_t h_ends[2] = {0, span};
      CS_HIP(hipMemcpyAsync(ends->p, h_ends, sizeof(h_ends), hipMemcpyHostToDevice, s));
      CS_HIP(hipStreamSynchronize(s));  // (h_ends is on the stack)
      cs_column last;
      borrow_rows(last, ptr<const uint8_t>(tail), span, ends, 1);
      locate_fields(last, parser, ptr<Field>(fields) + rows - 1, s);
    }
    cs_column in_text;
    borrow_rows(in_text, bytes, cr_in_memory ? n + 1 : n, starts, in_place);
    locate_fields(in_text, parser, ptr<Field>(fields), s);
  }
  Buf spans = dev_alloc(sizeof(Span) * (size_t)rows, s);
  hipLaunchKernelGGL(k_csv_spans, dim3(blocks_for(rows)), dim3(kBlock), 0, s, bytes, ptr<const int64_t>(starts), ptr<const Field>(fields), rows, in_place,
                     ptr<const uint8_t>(tail), ptr<Span>(spans));
  CS_HIP(hipGetLastError());
  return column_from_spans(spans->p, rows, (int)(flags & (cscsv::kSortLength | cscsv::kSortName)), s);
}

}  // namespace

extern "C" {

int cs_csv_tile_bytes(void) { return kTileBytes; }

int cs_column_from_csv_buffer(const void* bytes, int64_t nbytes, int on_device, unsigned column, unsigned lines, unsigned flags, cs_stream stream,
                              cs_column** out) {
  return guard([&] {
    if (!out || nbytes < 0 || (nbytes > 0 && !bytes)) fail(CS_ERR_INVALID_ARG, "from_csv: bad arguments");
    *out = nullptr;
    require_device();
    hipStream_t s = S(stream);
    if (on_device) {
      *out = csv_column(static_cast<const uint8_t*>(bytes), nbytes, false, column, lines, flags, s);
      return;
    }
    Buf text = dev_alloc((size_t)nbytes + 1, s);
    if (nbytes) CS_HIP(hipMemcpyAsync(text->p, bytes, (size_t)nbytes, hipMemcpyHostToDevice, s));
    CS_HIP(hipMemsetAsync(ptr<uint8_t>(text) + nbytes, '\r', 1, s));
    *out = csv_column(ptr<const uint8_t>(text), nbytes, true, column, lines, flags, s);
  });
}

int cs_column_from_csv(const char* path, unsigned column, unsigned lines, unsigned flags, cs_stream stream, cs_column** out) {
  std::vector<uint8_t> data;
  const int st = guard([&] {
    if (!out || !path) fail(CS_ERR_INVALID_ARG, "from_csv: bad arguments");
    *out = nullptr;
    FILE* fp = fopen(path, "rb");
    if (!fp) return;  // util.cu:45-49: a null instance
    fseek(fp, 0, SEEK_END);
    const long size = ftell(fp);
    fseek(fp, 0, SEEK_SET);
    if (size > 0) {
      data.resize((size_t)size);
      data.resize(fread(data.data(), 1, (size_t)size, fp));
    }
    fclose(fp);
  });
  if (st != CS_OK || data.size() < 2) return st;  // util.cu:54-58: fewer than 2 bytes, a null instance
  return cs_column_from_csv_buffer(data.data(), (int64_t)data.size(), 0, column, lines, flags, stream, out);
}

}  // extern "C"
