// contains_re / match_re / count_re: the row-wise kernels (list simulator, tagged DFA, the rows a stream launch put
// off), the host route scan<MODE> with its steps, and the three C entries.  The stream kernel is regex_stream.h's,
// instantiated here for MODE 0-2 and 7-9.  scan<MODE> is also how replace_re and findall count matches (regex_exec.h).
#include <hip/hip_runtime.h>

#include "cs_internal.h"
#include "regex_exec.h"
#include "regex_stream.h"

using namespace cs;
using namespace csdev;
using namespace cs::rx;

namespace cs {
bool count_class_runs(const cs_column* col, const int32_t* d_bits, const std::vector<int32_t>& bits, hipStream_t s, int32_t* results, int64_t* hits);
}

namespace {

// MODE 0 contains_re, 1 match, 2 count_re
template <bool SMALL, int MODE>
__global__ void k_regex_scan(RowSrc src, Launch L, uint8_t* __restrict__ out8, int32_t* __restrict__ out32,
                             unsigned long long* __restrict__ found) {
  extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
  Ctx c = setup(L, src.flags, smem);
  const ColView& in = src.in;
  const int64_t nblk = (in.rows + blockDim.x - 1) / blockDim.x;
  int hits = 0;
  for (int64_t blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
    int64_t r = blk * blockDim.x + threadIdx.x;
    if (r >= in.rows) continue;
    int v = 0;
    if (row_is_valid(in.validity, r)) {
      int64_t b = in.offsets[r];
      csvm::Vm<SMALL> vm(c.P, c.mem, c.stride, in.chars + b, (int)(in.offsets[r + 1] - b));
      if (MODE == 2) v = csvm::row_count_re(vm);
      else v = csvm::row_contains_re(vm, MODE == 1);
    }
    if (MODE == 2) out32[r] = v;
    else out8[r] = (uint8_t)v;
    hits += v > 0;
  }
  long long t = block_reduce_sum(hits);
  if (threadIdx.x == 0 && t) atomicAdd(found, (unsigned long long)t);
}

template <int MODE, bool IN_LDS, bool WIDE = false>
__global__ void __launch_bounds__(256) k_tdfa_scan(RowSrc src, TLaunch L, uint8_t* __restrict__ out8,
                                                   int32_t* __restrict__ out32,
                                                   unsigned long long* __restrict__ found) {
  extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
  TCtx c = tsetup<IN_LDS>(L, src.flags, smem);
  const ColView& in = src.in;
  const int64_t nblk = (in.rows + blockDim.x - 1) / blockDim.x;
  int hits = 0;
  for (int64_t blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
    int64_t r = blk * blockDim.x + threadIdx.x;
    if (r >= in.rows) continue;
    int v = 0;
    if (row_is_valid(in.validity, r)) {
      int64_t b = in.offsets[r];
      typename std::conditional<WIDE, cstd::TdfaWide, cstd::Tdfa>::type vm(c.D, c.P, in.chars + b, (int)(in.offsets[r + 1] - b));
      vm.wide_ok = (b & ~(int64_t)3) + cstd::Tdfa::kMaskBytes <= src.safe_end;
      if (MODE == 2) v = csvm::row_count_re(vm);
      else v = csvm::row_contains_re(vm, MODE == 1);
    }
    if (MODE == 2) out32[r] = v;
    else out8[r] = (uint8_t)v;
    hits += v > 0;
  }
  long long t = block_reduce_sum(hits);
  if (threadIdx.x == 0 && t) atomicAdd(found, (unsigned long long)t);
}
// the rows a stream launch put off (ScanStreamArgs::deferred): a thread a row, the generic executor on the row's bytes (staged in LDS)
template <int MODE>
__global__ void __launch_bounds__(256) k_tdfa_scan_list(RowSrc src, TLaunch L, const int32_t* __restrict__ list, const unsigned* __restrict__ nlist, unsigned cap,
                                                        uint8_t* __restrict__ out8, int32_t* __restrict__ out32, unsigned long long* __restrict__ found) {
  extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
  const unsigned total = min(*nlist, cap);
  if ((unsigned)blockIdx.x * 256u >= total) return;  // (nothing for this workgroup: not even the tables)
  TCtx c = tsetup<true>(L, src.flags, smem);
  const ColView& in = src.in;
  int hits = 0;
  for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < total; i += gridDim.x * 256u) {
    const int64_t r = list[i];
    const int64_t b = in.offsets[r];
    const int n = (int)(in.offsets[r + 1] - b);
    uint8_t* buf = reinterpret_cast<uint8_t*>(smem) + (((size_t)L.tdfa_words * 4 + 15) & ~(size_t)15) + (size_t)threadIdx.x * kListRowBytes;
    const uint8_t* p = list_row_to_lds(in.chars + b, n, buf, in.chars, in.chars + src.safe_end);
    cstd::Tdfa vm(c.D, c.P, p, n);
    vm.wide_ok = p != in.chars + b || (b & ~(int64_t)3) + cstd::Tdfa::kMaskBytes <= src.safe_end;
    const int v = MODE == 2 ? csvm::row_count_re(vm) : csvm::row_contains_re(vm, false);
    if (MODE == 2) out32[r] = v;
    else out8[r] = (uint8_t)v;
    hits += v > 0;
  }
  const long long t = block_reduce_sum(hits);
  if (threadIdx.x == 0 && t) atomicAdd(found, (unsigned long long)t);
}

__global__ void k_counts_to_flags(const int32_t* __restrict__ counts, int64_t rows, uint8_t* __restrict__ flags) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r < rows) flags[r] = counts[r] > 0 ? 1 : 0;
}

// ---- contains_re / match_re / count_re: the host route ------------------------------------------------------------------
// scan<MODE> (MODE 0 contains_re, 1 match_re, 2 count_re) runs a ScanCall as the sequence it is -- the column's pieces,
// contains by counts, class runs, the stream kernel and the rows it put off, the row-wise kernels -- each step a function
// that says whether it took the call.  The stream kernel in turn: its FORM (scan_form: which variant runs, on how much
// LDS), the KERNEL (scan_stream_kernel: the one place that names the instantiations) and the LAUNCH (scan_stream).
// Several questions below launch kernels or wait on the stream the first time they are asked of a column (pieces_for,
// sample_has_high_bytes, odd_rows_few, max_row_bytes, bits_route, candidate_share, choose_tile): the order of the `&&`
// chains decides whether they are asked at all.  Keep it.

// A column with rows beyond the 96-bit masks, white space a safe cut for the program (pieces_for): the pieces' flags or
// counts, folded into the rows' (cs_virtual.hip).  Not match_re: it looks at a row's start only.
template <int MODE>
bool scan_on_pieces(const ScanCall& c) {
  if (MODE == 1) return false;
  const VirtualRows* vr = pieces_for(c.col, c.re, c.s, false, MODE == 0);
  if (!vr) return false;
  const cs_column* pc = vr->col.get();
  Buf piece_res = dev_alloc(c.esz * (size_t)pc->rows, c.s);
  scan<MODE>(ScanCall{pc, c.re, piece_res->p, c.esz, 1, c.s, nullptr, c.name});
  note_route_pieces();
  const ResultsOut res(c.results, c.esz * (size_t)c.col->rows, c.on_device, c.s);
  const int64_t hits = MODE == 2 ? virtual_reduce_i32(vr, ptr<const int32_t>(piece_res), c.col->rows, static_cast<int32_t*>(res.dev), c.s)
                                 : virtual_reduce_u8(vr, ptr<const uint8_t>(piece_res), c.col->rows, static_cast<uint8_t*>(res.dev), c.s);
  if (!c.on_device) res.finish(c.s);  // (the reduction brought its count back: a device caller's results are complete)
  if (c.found) *c.found = hits;
  return true;
}

// contains_re of a program with a unit decomposition whose candidate bytes are most of the column (`\w+@\w+` on log lines):
// the row lanes' scan restarts at every candidate -- 9.0 ms on the C3 column where count_re, on the unit scan, takes 1.9.
// "Holds a match" is "counts at least one": the unit scan's counts, turned into flags.
template <int MODE>
bool contains_by_counts(const ScanCall& c) {
  const cs_column* col = c.col;
  cs_regex* re = c.re;
  const hipStream_t s = c.s;
  if (!(MODE == 0 && use_tdfa(re) && (re->tdfa[31] & 1) && ((re->tdfa[30] >> 16) & 15) == 0 && !cs::cfg("CS_NO_CONTAINS_BY_COUNT") && !cs::cfg("CS_REGEX_ROWWISE") &&
        !cs::cfg("CS_NO_UNITS") && (((re->tdfa[31] >> 17) & 3) != 0 || !sample_has_high_bytes(col, s) || odd_rows_few(col, s)) && max_row_bytes(col, s) + 3 <= cstd::Tdfa::kMaskBytes &&
        !bits_route(re, col, s, BITS_CONTAINS, odd_rows_few(col, s)) && !bits_route(re, col, s, BITS_COUNT, odd_rows_few(col, s)) &&
        candidate_share(re, col, s) >= 0.5))
    return false;
  Buf counts = dev_alloc(sizeof(int32_t) * (size_t)col->rows, s);
  int64_t hits = 0;
  scan<2>(ScanCall{col, re, counts->p, sizeof(int32_t), 1, s, &hits, c.name});
  const ResultsOut flags(c.results, (size_t)col->rows, c.on_device, s);
  hipLaunchKernelGGL(k_counts_to_flags, dim3(blocks_for(col->rows)), dim3(256), 0, s, ptr<const int32_t>(counts), col->rows, static_cast<uint8_t*>(flags.dev));
  CS_HIP(hipGetLastError());
  flags.finish(s);
  if (c.found) *c.found = hits;
  return true;
}

// count_re of ONE class, once or in a `+` loop, on a column the 96-bit-mask forms do not take (long rows, non-ASCII text) and
// whose candidates are everywhere: the byte-parallel size pass of cs_runs.hip counting matches -- count_re(\w+), the words of
// a row, on the C5 column: 15.8 ms on the long-row automaton form
template <int MODE>
bool count_by_class_runs(const ScanCall& c, const ResultsOut& res) {
  const cs_column* col = c.col;
  cs_regex* re = c.re;
  const hipStream_t s = c.s;
  if (MODE != 2 || re->bits.empty() || !(re->bits[2] & (csbits::F_BYTE_CLASS | csbits::F_FLAG_CLASS))) return false;
  upload(re, s);
  const TileChoice tc0 = choose_tile(col, s, true);
  const bool masks_form = tc0.R == 64 && !tc0.lng && (!sample_has_high_bytes(col, s) || odd_rows_few(col, s));
  const bool chain_there = !re->tdfa.empty() && ((re->tdfa[30] >> 16) & 15) != 0 && tc0.R == 64 && !tc0.lng;
  const bool flag_class = (re->bits[2] & csbits::F_BYTE_CLASS) == 0;
  int64_t hits = 0;
  if (!(re->d_bits && (cs::cfg("CS_CLASS_RUNS_ALWAYS") || (!masks_form && !(flag_class && chain_there) && candidate_share(re, col, s) >= 0.05)) &&
        count_class_runs(col, ptr<const int32_t>(re->d_bits), re->bits, s, static_cast<int32_t*>(res.dev), &hits)))
    return false;
  note_route("runs");
  if (!c.on_device) res.finish(s);  // (as on the pieces: the pass brought its count back)
  if (c.found) *c.found = hits;
  return true;
}

struct ScanRun {  // a call and what its launches share
  const ScanCall& c;
  bool tdfa, wide;            // the tagged DFA runs the program; ... with five to eight live threads (TdfaWide on the same kernels' generic row path)
  TPlan tp;                   // (tdfa || wide)
  Plan pl;                    // (neither: the list simulator)
  void* out;                  // the rows' results on the device (ResultsOut::dev)
  unsigned long long* found;  // the zeroed count the kernels add to
  RowSrc src;
};
// The kernels take a flags pointer and a counts pointer: the one MODE means is the results buffer, the other null.
template <int MODE>
uint8_t* out8_of(const ScanRun& r) {
  return MODE == 2 ? nullptr : static_cast<uint8_t*>(r.out);
}
template <int MODE>
int32_t* out32_of(const ScanRun& r) {
  return MODE == 2 ? static_cast<int32_t*>(r.out) : nullptr;
}

// Which variant of k_tdfa_scan_stream runs, and on how much LDS.
struct ScanForm {
  // a column whose sample holds a few bytes >= 0x80: the rows that hold them are put off -- ScanStreamArgs::deferred,
  // k_tdfa_scan_list -- and the forms are chosen as on plain ASCII; the C5 column, one row in 170: contains_re of the gtest
  // pattern 9.9 ms when every sub-tile with such a row went to the row-by-row scan
  bool put_off;
  // the unit scan (k_tdfa_scan_stream<.., UNITS>): patterns whose tagged DFA offers the decomposition, rows within the masks
  // (count_re only: contains_re stops at a row's first match, and scanning every unit of the row cost more than the
  // balance won -- 3.87 against 2.66 ms on the 100M-row C3 column)
  // (... but the unit form of the kernel is taken for contains_re too when the pattern lets the unit route serve tiles with
  // bytes >= 0x80 -- header word 31 bits 17 / 18 -- and a sample of the chars holds such bytes: ASCII tiles keep the row
  // lanes' scan inside it, at a few per cent more than the plain form)
  // (chain patterns -- header words 29 / 30 -- were tried on the unit form for contains_re as well: 2.18 against 2.10 ms; the
  // plain form's first-match scan stays)
  // (a chain pattern without a unit decomposition -- one with a suffix, regex_tdfa.cpp -- takes the same kernels: their unit
  // routes test header word 31 bit 0 themselves)
  bool units;
  // the bit-parallel form (regex_bits.h): contains_re / count_re of patterns whose candidates are everywhere
  bool bits_form;
  int bits_k;
  size_t bits_lds;
  // a chain pattern on a column whose sample is plain ASCII: count_re by the chain's arithmetic
  bool chain_scan;
  // (a chain's arithmetic reads no table: where the tables cost the launch a workgroup per CU -- four fit in 40 KB each --
  // they stay in memory, as in cs_replace_re)
  // (the bit form is such a form too: its sub-tiles of plain ASCII never touch the automaton)
  bool chain_global;
  bool wide;        // (ScanRun::wide)
  size_t scan_tbl;  // bytes of the automaton's tables in LDS: all of them, or -- chain_global -- header + tail words (tsetup)
  size_t lds;       // dynamic LDS of a workgroup; beyond 150 KB there is no stream launch
  const char* note;  // cs_debug_last_route
  ScanStreamKernel kern;
};

// The instantiation of k_tdfa_scan_stream a form runs on: every one the scans hold is named here, once, from the plainest
// form on.  The parameters are <MODE, IN_LDS, LONG, UNITS, CHAIN, BITS> (their meaning: at the kernel); MODE + 7 is the
// WIDE executor.  match_re has the plain and wide forms only; the unit, chain and bit forms are count_re's and contains_re's.
template <int MODE>
ScanStreamKernel scan_stream_kernel(const ScanForm& f, bool lng) {
  constexpr int M = MODE == 2 ? 2 : 0;
  if (!f.wide && !f.units && !f.bits_form) return lng ? &k_tdfa_scan_stream<MODE, true, true> : &k_tdfa_scan_stream<MODE, true, false>;
  if (f.units && !f.chain_scan && !f.bits_form) return &k_tdfa_scan_stream<M, true, false, true>;
  if (f.chain_scan) {
    if (!f.chain_global) return &k_tdfa_scan_stream<2, true, false, true, true>;
    return &k_tdfa_scan_stream<2, false, false, true, true>;
  }
  if (f.bits_form) return f.chain_global ? &k_tdfa_scan_stream<M, false, false, true, true, true> : &k_tdfa_scan_stream<M, true, false, true, true, true>;
  return lng ? &k_tdfa_scan_stream<MODE + 7, true, true> : &k_tdfa_scan_stream<MODE + 7, true, false>;
}

template <int MODE>
ScanForm scan_form(const ScanRun& r, const TileChoice& tc) {
  const cs_column* col = r.c.col;
  const cs_regex* re = r.c.re;
  const hipStream_t s = r.c.s;
  const int cap = tc.cap;
  ScanForm f{};
  f.wide = r.wide;
  f.put_off = (MODE == 0 || MODE == 2) && !f.wide && !tc.lng && tc.R == 64 && sample_has_high_bytes(col, s) && odd_rows_few(col, s);
  const bool high_sample = sample_has_high_bytes(col, s) && !f.put_off;
  f.units = !f.wide && (MODE == 2 || (MODE == 0 && ((re->tdfa[31] >> 17) & 3) != 0 && high_sample)) &&
            ((re->tdfa[31] & 1) != 0 || (MODE == 2 && ((re->tdfa[30] >> 16) & 15) != 0)) &&
            !tc.lng && tc.R == 64 && !cs::cfg("CS_NO_UNITS");
  f.bits_form = !f.wide && (MODE == 0 || MODE == 2) && !tc.lng && tc.R == 64 && bits_route(re, col, s, MODE == 2 ? BITS_COUNT : BITS_CONTAINS, f.put_off);
  f.bits_k = f.bits_form ? std::max(re->bits[1], 2) : 0;
  f.bits_lds = f.bits_form ? (size_t)bits_lds_bytes((int)re->bits.size()) : 0;
  f.lds = f.bits_form ? r.tp.lds_bytes + f.bits_lds + (size_t)(cap + 32 + f.bits_k * ((cap >> 3) + 32) + kUnitQueue * 4 + 64 * 4 + 16) * 4
                      : r.tp.lds_bytes + (size_t)(cap + 32 + (cap >> 3) + 32 + (f.units ? (cap >> 3) + 32 + kUnitQueue * 4 + 64 * 4 + 16 : 0)) * 4;
  if (f.put_off) f.lds += (size_t)((cap >> 3) + 32 + 64 * 4) * 4;  // (the bitmap of such bytes and the rows waiting for the list, a wave)
  f.chain_scan = f.units && MODE == 2 && !f.bits_form && ((re->tdfa[30] >> 16) & 15) != 0 && !high_sample && !cs::cfg("CS_NO_CHAIN_FORM");
  f.chain_global = (f.chain_scan || f.bits_form) && f.lds > 40 * 1024 && f.lds - r.tp.lds_bytes + cstd::kHeadTailWords * 4 <= 40 * 1024 && !cs::cfg("CS_CHAIN_TABLES_IN_LDS");
  f.scan_tbl = f.chain_global ? (size_t)cstd::kHeadTailWords * 4 : r.tp.lds_bytes;
  if (f.chain_global) f.lds -= r.tp.lds_bytes - f.scan_tbl;
  f.note = f.bits_form ? "bits" : f.wide ? "wide" : f.chain_scan ? "chain" : f.units ? "units" : "plain";
  f.kern = scan_stream_kernel<MODE>(f, tc.lng);
  return f;
}

// The rows a stream launch put off: the list kernel, a thread a row.  More such rows than the sample promised and the
// list holds: the count is zeroed again, the call is not taken and the column is scanned once more, row-wise, with
// nothing put off.
template <int MODE>
bool scan_put_off_rows(const ScanRun& r, const ScanStreamArgs& sa, const Buf& later, const Buf& nlater) {
  const hipStream_t s = r.c.s;
  note_route_put_off();
  const unsigned lgrid = (unsigned)std::min<int64_t>(((int64_t)sa.deferred_cap + 255) / 256, 2048);
  const size_t list_lds = r.tp.lds_bytes + (size_t)256 * kListRowBytes;  // (the tables and a row a thread)
  if (list_lds > 48 * 1024)
    CS_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_tdfa_scan_list<MODE == 2 ? 2 : 0>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)list_lds));
  ProfScope ps("k_tdfa_scan_list", s);
  hipLaunchKernelGGL((k_tdfa_scan_list<MODE == 2 ? 2 : 0>), dim3(lgrid), dim3(256), list_lds, s, r.src, r.tp.d, ptr<const int32_t>(later), ptr<const unsigned>(nlater),
                     sa.deferred_cap, out8_of<MODE>(r), out32_of<MODE>(r), r.found);
  unsigned* hn = (unsigned*)pinned_scratch(sizeof(unsigned));
  CS_HIP(hipMemcpyAsync(hn, nlater->p, sizeof(unsigned), hipMemcpyDeviceToHost, s));
  CS_HIP(hipStreamSynchronize(s));
  if (*hn <= sa.deferred_cap) return true;
  note_fallback("regex-deferred-rows-overflow");
  CS_HIP(hipMemsetAsync(r.found, 0, 8, s));
  return false;
}

// The stream kernel: row tiles through LDS on a persistent grid, for a tagged DFA whose tables fit LDS.
template <int MODE>
bool scan_stream(const ScanRun& r) {
  const cs_column* col = r.c.col;
  const cs_regex* re = r.c.re;
  const hipStream_t s = r.c.s;
  if (!r.tdfa || !r.tp.d.in_lds || cs::cfg("CS_REGEX_ROWWISE")) return false;
  const TileChoice tc = choose_tile(col, s);
  const ScanForm f = scan_form<MODE>(r, tc);
  if (!tc.R || f.lds > 150 * 1024) return false;
  ScanStreamArgs sa = stream_args(col, r.tp, tc);
  if (f.chain_global) sa.L.in_lds = 2;
  sa.out8 = out8_of<MODE>(r);
  sa.out32 = out32_of<MODE>(r);
  sa.found = r.found;
  sa.tbl_bytes = (int)(f.scan_tbl + f.bits_lds);
  sa.bits = f.bits_form ? ptr<const int32_t>(re->d_bits) : nullptr;
  sa.bits_off = (int)f.scan_tbl;
  sa.bits_words = f.bits_form ? (int)re->bits.size() : 0;
  sa.bits_k = f.bits_form ? re->bits[1] : 0;
  note_route(f.note);
  Buf later, nlater;
  if (f.put_off) {
    sa.deferred_cap = (unsigned)std::min<int64_t>(col->rows, col->rows / 8 + 4096);
    later = dev_alloc(sizeof(int32_t) * (size_t)sa.deferred_cap, s);
    nlater = dev_alloc(sizeof(unsigned), s);
    CS_HIP(hipMemsetAsync(nlater->p, 0, sizeof(unsigned), s));
    sa.deferred = ptr<int32_t>(later);
    sa.ndeferred = ptr<unsigned>(nlater);
  }
  {
    ProfScope ps(r.c.name, s);
    launch_resident(f.kern, f.lds, (sa.nsub + 3) / 4, s, sa);
  }
  return !f.put_off || scan_put_off_rows<MODE>(r, sa, later, nlater);
}

// The row-wise kernels, a thread a row: the tagged DFA (wide or not, tables in LDS or in memory) or the list simulator.
template <int MODE>
void scan_rowwise(const ScanRun& r) {
  const hipStream_t s = r.c.s;
  const TPlan& tp = r.tp;
  const Plan& pl = r.pl;
  uint8_t* out8 = out8_of<MODE>(r);
  int32_t* out32 = out32_of<MODE>(r);
  ProfScope ps(r.c.name, s);
  if (r.wide)
    if (tp.d.in_lds)
      hipLaunchKernelGGL((k_tdfa_scan<MODE, true, true>), dim3(tp.grid), dim3(256), tp.lds_bytes, s, r.src, tp.d, out8, out32, r.found);
    else
      hipLaunchKernelGGL((k_tdfa_scan<MODE, false, true>), dim3(tp.grid), dim3(256), 0, s, r.src, tp.d, out8, out32, r.found);
  else if (r.tdfa)
    if (tp.d.in_lds)
      hipLaunchKernelGGL((k_tdfa_scan<MODE, true>), dim3(tp.grid), dim3(256), tp.lds_bytes, s, r.src, tp.d, out8, out32, r.found);
    else
      hipLaunchKernelGGL((k_tdfa_scan<MODE, false>), dim3(tp.grid), dim3(256), 0, s, r.src, tp.d, out8, out32, r.found);
  else if (pl.small)
    hipLaunchKernelGGL((k_regex_scan<true, MODE>), dim3(pl.grid), dim3(pl.threads), pl.lds_bytes, s, r.src, pl.d, out8, out32, r.found);
  else
    hipLaunchKernelGGL((k_regex_scan<false, MODE>), dim3(pl.grid), dim3(pl.threads), pl.lds_bytes, s, r.src, pl.d, out8, out32, r.found);
}

}  // namespace

template <int MODE>
void cs::rx::scan(const ScanCall& c) {
  const cs_column* col = c.col;
  const hipStream_t s = c.s;
  if (c.found) *c.found = 0;
  note_route("");
  if (col->rows == 0) return;
  if (scan_on_pieces<MODE>(c)) return;
  if (contains_by_counts<MODE>(c)) return;
  const bool wide = use_tdfa_wide(c.re);
  const bool tdfa = use_tdfa(c.re) || wide;
  Plan pl{};
  TPlan tp{};
  if (tdfa) tp = tplan(c.re, col->rows, s);
  else pl = plan(c.re, col->rows, s);
  const ResultsOut res(c.results, c.esz * (size_t)col->rows, c.on_device, s);  // (before the class-runs attempt; the count after it)
  if (count_by_class_runs<MODE>(c, res)) return;
  const Buf cnt = zeroed_count(s);
  const ScanRun r{c, tdfa, wide, tp, pl, res.dev, ptr<unsigned long long>(cnt), row_src(col)};
  if (!scan_stream<MODE>(r)) scan_rowwise<MODE>(r);
  CS_HIP(hipGetLastError());
  res.copy_back(s);
  const int64_t n = read_count(cnt, s);
  if (c.found) *c.found = n;
}
// (the callers in the other unit, cs_regex.hip: count_matches_first, findall_count_rows)
template void cs::rx::scan<0>(const ScanCall&);
template void cs::rx::scan<1>(const ScanCall&);
template void cs::rx::scan<2>(const ScanCall&);

extern "C" {

// NVStrings::contains_re -- count.cu:59-110
int cs_contains_re(const cs_column* col, const cs_regex* re, uint8_t* results, int on_device, cs_stream stream,
                   int64_t* found) {
  return guard([&] {
    if (found) *found = -1;
    if (!col || !re || !results) fail(CS_ERR_INVALID_ARG, "contains_re: null argument");
    scan<0>(ScanCall{col, const_cast<cs_regex*>(re), results, sizeof(uint8_t), on_device, S(stream), found, "k_contains_re"});
  });
}
// NVStrings::match -- count.cu:113-165
int cs_match_re(const cs_column* col, const cs_regex* re, uint8_t* results, int on_device, cs_stream stream,
                int64_t* found) {
  return guard([&] {
    if (found) *found = -1;
    if (!col || !re || !results) fail(CS_ERR_INVALID_ARG, "match: null argument");
    scan<1>(ScanCall{col, const_cast<cs_regex*>(re), results, sizeof(uint8_t), on_device, S(stream), found, "k_match_re"});
  });
}
// NVStrings::count_re -- count.cu:168-250
int cs_count_re(const cs_column* col, const cs_regex* re, int32_t* results, int on_device, cs_stream stream,
                int64_t* found) {
  return guard([&] {
    if (found) *found = -1;
    if (!col || !re || !results) fail(CS_ERR_INVALID_ARG, "count_re: null argument");
    scan<2>(ScanCall{col, const_cast<cs_regex*>(re), results, sizeof(int32_t), on_device, S(stream), found, "k_count_re"});
  });
}

}  // extern "C"
