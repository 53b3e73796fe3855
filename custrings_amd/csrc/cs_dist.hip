// The distributed NVCategory build behind the C ABI (BASELINE.json north_star: local build -> exchange of the ranks'
// sorted key sets over RCCL -> merge -> remap; the reference itself is single-GPU, the merge semantics are
// NVCategory::create_from_categories, NVCategory.cu:430-514).  One process per GPU; nothing else on the hot path
// exchanges data.  custrings_amd/dist.py does the same through torch.distributed; this is what a C++ consumer of
// libNVCategory.so calls with the ncclComm_t it already has.
//
// Two routes, chosen from the ranks' key counts (the first exchange):
//   * all-gather of the key sets, padded to the largest, every rank merges all of them (K far below N);
//   * from kPartitionMinKeys keys in all (K close to N: BASELINE.json C4 lists K = 100M) the merge is partitioned by key
//     RANGE -- splitters from a sample, an all-to-all of every key to its range's owner, an all-gather of the merged
//     ranges: every rank merges 1/G of the keys instead of all of them (merge_partitioned below).
//
// RCCL is looked up in the process at run time (dlsym on what is loaded, else dlopen of librccl.so): the communicator
// belongs to the CALLER's RCCL, and a process that never builds a distributed category needs no RCCL at all (the CPU
// test box loads this library without a GPU runtime behind it).
#include <dlfcn.h>
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <vector>

#include "cs_internal.h"

using namespace cs;


namespace {

// ncclAllGather(const void* sendbuff, void* recvbuff, size_t sendcount, ncclDataType_t, ncclComm_t, hipStream_t); ncclUint8 = 1
typedef int (*nccl_allgather_t)(const void*, void*, size_t, int, void*, hipStream_t);
typedef int (*nccl_sendrecv_t)(void*, size_t, int, int, void*, hipStream_t);  // ncclSend (const void*) / ncclRecv: buff, count, type, peer, comm, stream
typedef int (*nccl_group_t)();
typedef const char* (*nccl_errstr_t)(int);
nccl_allgather_t g_allgather = nullptr;
nccl_sendrecv_t g_send = nullptr, g_recv = nullptr;
nccl_group_t g_group_start = nullptr, g_group_end = nullptr;
nccl_errstr_t g_errstr = nullptr;
void resolve_rccl() {
  static std::once_flag once;
  std::call_once(once, [] {
    void* lib = nullptr;
    auto find = [&](const char* name) -> void* {
      void* sym = dlsym(RTLD_DEFAULT, name);
      if (!sym && !lib) {
        for (const char* so : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
          lib = dlopen(so, RTLD_NOW | RTLD_GLOBAL);
          if (lib) break;
        }
      }
      if (!sym && lib) sym = dlsym(lib, name);
      return sym;
    };
    g_allgather = reinterpret_cast<nccl_allgather_t>(find("ncclAllGather"));
    g_send = reinterpret_cast<nccl_sendrecv_t>(find("ncclSend"));
    g_recv = reinterpret_cast<nccl_sendrecv_t>(find("ncclRecv"));
    g_group_start = reinterpret_cast<nccl_group_t>(find("ncclGroupStart"));
    g_group_end = reinterpret_cast<nccl_group_t>(find("ncclGroupEnd"));
    g_errstr = reinterpret_cast<nccl_errstr_t>(find("ncclGetErrorString"));
  });
}
void rccl_check(int rc, const char* what) {
  if (rc != 0) fail(CS_ERR_INTERNAL, std::string(what) + ": " + (g_errstr ? g_errstr(rc) : "error"));
}
int rccl_allgather(void* comm, const void* send, void* recv, size_t bytes, void* stream) {
  rccl_check(g_allgather(send, recv, bytes, /* ncclUint8 */ 1, comm, static_cast<hipStream_t>(stream)), "ncclAllGather");
  return 0;
}
// the all-to-all of variable pieces as one group of point-to-point operations (xGMI is point to point: every pair its own link)
int rccl_alltoallv(void* comm, const void* send, const size_t* send_bytes, const size_t* send_off, void* recv, const size_t* recv_bytes, const size_t* recv_off,
                   int nranks, void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  rccl_check(g_group_start(), "ncclGroupStart");
  // (an error inside the group is remembered, the group is CLOSED whatever happened -- an open group would stay on the
  // caller's communicator -- and only then reported)
  int first = 0;
  const char* where = "";
  for (int d = 0; d < nranks && first == 0; ++d) {
    if (send_bytes[d]) {
      first = g_send(const_cast<uint8_t*>(static_cast<const uint8_t*>(send)) + send_off[d], send_bytes[d], 1, d, comm, s);
      where = "ncclSend";
    }
    if (first == 0 && recv_bytes[d]) {
      first = g_recv(static_cast<uint8_t*>(recv) + recv_off[d], recv_bytes[d], 1, d, comm, s);
      where = "ncclRecv";
    }
  }
  const int end = g_group_end();
  rccl_check(first, where);
  rccl_check(end, "ncclGroupEnd");
  return 0;
}

struct KeyHeader {  // what every rank tells the others about a column it contributes
  int64_t keys, bytes, null_first;
  int64_t status;  // 0, or the status of a failure on that rank: every rank still takes part in this exchange and all stop together
};

struct Exchange {
  cs_allgather_fn allgather;
  cs_alltoallv_fn alltoallv;  // may be null: the all-gather route only
  void* ctx;
  int nranks, rank;
  hipStream_t s;
};

bool null_first_of(const cs_column* c, hipStream_t s) {  // (the null key, if any, is key 0)
  if (!c || c->rows == 0 || !c->validity) return false;
  uint8_t first = 0xFF;
  CS_HIP(hipMemcpyAsync(&first, c->validity->p, 1, hipMemcpyDeviceToHost, s));
  CS_HIP(hipStreamSynchronize(s));
  return !(first & 1);
}
// What a throw on this rank becomes: a status and its text, carried to the next exchange, where all ranks stop together
struct Failure {
  int status = 0;
  std::string why;
};
template <class F>
Failure caught(F&& work) {
  try {
    work();
  } catch (const Error& e) {
    return {e.code ? e.code : CS_ERR_INTERNAL, e.msg};
  } catch (const std::exception& e) {
    return {CS_ERR_INTERNAL, e.what()};
  }
  return {};
}
// One record of int64 words per rank: this rank's `mine` out, every rank's records back on the host (rank r's at word
// mine.size() * r).  `failed`: what to say when the transport fails.
std::vector<int64_t> exchange_records(const Exchange& x, const std::vector<int64_t>& mine, const std::string& failed) {
  hipStream_t s = x.s;
  const size_t n = (size_t)x.nranks, row = sizeof(int64_t) * mine.size();
  Buf d = dev_alloc(row * (n + 1), s);  // (small: a failure here is the exchange's own)
  uint8_t* d_mine = ptr<uint8_t>(d) + row * n;
  CS_HIP(hipMemcpyAsync(d_mine, mine.data(), row, hipMemcpyHostToDevice, s));
  CS_HIP(hipStreamSynchronize(s));  // (`mine` is pageable)
  if (x.allgather(x.ctx, d_mine, d->p, row, s) != 0) fail(CS_ERR_INTERNAL, "category_build_distributed: " + failed);
  std::vector<int64_t> all(mine.size() * n);
  CS_HIP(hipMemcpyAsync(all.data(), d->p, row * n, hipMemcpyDeviceToHost, s));
  CS_HIP(hipStreamSynchronize(s));
  return all;
}
// The last word of every rank's record (`words` each) is its status.  When any rank has failed ALL ranks stop here
// together: this one with its own error when it has one and `own_stage` is given (without: the caller reports it, see
// headers_or_own_failure), the others naming the first rank that failed.
void stop_if_failed(const std::vector<int64_t>& records, size_t words, const Failure& own, const char* own_stage, const char* when, const char* what) {
  if (own.status && own_stage) fail(own.status, own.why + " (" + own_stage + "; every rank stops)");
  for (size_t r = 0; r * words < records.size(); ++r) {
    const int64_t st = records[words * r + words - 1];
    if (st != 0)
      fail(st == CS_ERR_ALLOC ? CS_ERR_ALLOC : CS_ERR_INTERNAL,
           "category_build_distributed: rank " + std::to_string(r) + " failed" + when + " (status " + std::to_string(st) + ", " + what + "); every rank stops");
  }
}
// one fixed-size record per rank; a rank that failed locally says so and every rank fails with it
std::vector<KeyHeader> gather_headers(const Exchange& x, const cs_column* mine, int status, const char* what) {
  const KeyHeader me{mine ? mine->rows : 0, mine ? mine->nbytes : 0, status == 0 && null_first_of(mine, x.s) ? 1 : 0, status};
  const std::vector<int64_t> records = exchange_records(x, {me.keys, me.bytes, me.null_first, me.status}, std::string("the exchange of the sizes failed (") + what + ")");
  stop_if_failed(records, 4, Failure{}, nullptr, " before the exchange", what);
  std::vector<KeyHeader> all(x.nranks);
  memcpy(all.data(), records.data(), sizeof(KeyHeader) * all.size());
  if (all[x.rank].keys != me.keys || all[x.rank].bytes != me.bytes) fail(CS_ERR_INTERNAL, "category_build_distributed: the exchange returned another rank's record at this rank's place");
  return all;
}
// ... or, when this rank had failed before and the exchange says so (or fails itself), this rank's own failure
std::vector<KeyHeader> headers_or_own_failure(const Exchange& x, const cs_column* mine, const Failure& own, const char* what) {
  try {
    return gather_headers(x, own.status ? nullptr : mine, own.status, what);
  } catch (const Error& e) {
    if (own.status) fail(own.status, own.why + " (" + e.msg + ")");
    throw;
  }
}
// An agreement point: every rank contributes its status word, and when any rank has failed since the last exchange ALL
// ranks stop here together -- the one that failed with its own error, the others naming it -- instead of one rank
// throwing while its peers wait in the next collective for ever.
void agree(const Exchange& x, const Failure& own, const char* stage) {
  stop_if_failed(exchange_records(x, {own.status}, std::string("the status exchange failed (") + stage + ")"), 1, own, stage, "", stage);
}
// the validity of a key set whose key 0 is the null key: all valid, row 0 null
Buf null_first_mask(int64_t keys, hipStream_t s) {
  Buf v = dev_alloc(validity_bytes(keys), s);
  CS_HIP(hipMemsetAsync(v->p, 0xFF, validity_bytes(keys), s));
  CS_HIP(hipMemsetAsync(v->p, 0xFE, 1, s));
  return v;
}
// One all-to-all of `elem`-byte elements.  `send_at` and `recv_at` hold nranks + 1 element positions: peer d is sent the
// elements send_at[d] .. send_at[d + 1] (`send` points at element send_at[0]), and what it sends lands at the elements
// recv_at[d] .. recv_at[d + 1] of `recv`.
void exchange_slices(const Exchange& x, const void* send, const std::vector<int64_t>& send_at, void* recv, const std::vector<int64_t>& recv_at, size_t elem, const char* what) {
  const int n = x.nranks;
  std::vector<size_t> send_bytes(n), send_off(n), recv_bytes(n), recv_off(n);
  for (int d = 0; d < n; ++d) {
    send_bytes[d] = elem * (size_t)(send_at[d + 1] - send_at[d]);
    send_off[d] = elem * (size_t)(send_at[d] - send_at[0]);
    recv_bytes[d] = elem * (size_t)(recv_at[d + 1] - recv_at[d]);
    recv_off[d] = elem * (size_t)(recv_at[d] - recv_at[0]);
  }
  if (x.alltoallv(x.ctx, send, send_bytes.data(), send_off.data(), recv, recv_bytes.data(), recv_off.data(), n, x.s) != 0)
    fail(CS_ERR_INTERNAL, std::string("category_build_distributed: the all-to-all of the ") + what + " failed");
}

// Every rank's column on every rank: offsets and chars padded to the largest (an all-gather moves equal pieces); the
// columns are views into the two gathered buffers.
struct Gathered {
  std::vector<KeyHeader> hdr;
  std::vector<std::unique_ptr<cs_column>> cols;
  Buf offs, chrs;
  int64_t total_keys = 0;
  std::vector<const cs_column*> ptrs() const {
    std::vector<const cs_column*> v;
    for (const auto& c : cols) v.push_back(c.get());
    return v;
  }
};
Gathered gather_columns(const Exchange& x, const cs_column* mine, std::vector<KeyHeader> hdr, const char* what) {
  hipStream_t s = x.s;
  const int n = x.nranks;
  Gathered g;
  g.hdr = std::move(hdr);
  int64_t max_keys = 0, max_bytes = 0;
  for (const KeyHeader& h : g.hdr) {
    max_keys = std::max(max_keys, h.keys);
    max_bytes = std::max(max_bytes, h.bytes);
    g.total_keys += h.keys;
  }
  const KeyHeader& me = g.hdr[x.rank];
  const size_t off_piece = sizeof(int64_t) * (size_t)(max_keys + 1), chr_piece = (size_t)((max_bytes + 15) & ~(int64_t)15);
  // (the gathered buffers hold every rank's piece: a rank that cannot have them says so before anybody enters the all-gather)
  agree(x, caught([&] {
          g.offs = dev_alloc(off_piece * (n + 1), s);
          g.chrs = dev_alloc(chr_piece * (n + 1) + 16, s);
        }),
        what);
  uint8_t* my_off = ptr<uint8_t>(g.offs) + off_piece * n;
  uint8_t* my_chr = ptr<uint8_t>(g.chrs) + chr_piece * n;
  CS_HIP(hipMemsetAsync(my_off, 0, off_piece, s));
  if (me.keys > 0) CS_HIP(hipMemcpyAsync(my_off, mine->d_offsets(), sizeof(int64_t) * (size_t)(me.keys + 1), hipMemcpyDeviceToDevice, s));
  if (me.bytes > 0) CS_HIP(hipMemcpyAsync(my_chr, mine->d_chars(), (size_t)me.bytes, hipMemcpyDeviceToDevice, s));
  if (x.allgather(x.ctx, my_off, g.offs->p, off_piece, s) != 0) fail(CS_ERR_INTERNAL, std::string("category_build_distributed: the exchange of the offsets failed (") + what + ")");
  if (chr_piece && x.allgather(x.ctx, my_chr, g.chrs->p, chr_piece, s) != 0)
    fail(CS_ERR_INTERNAL, std::string("category_build_distributed: the exchange of the bytes failed (") + what + ")");
  for (int r = 0; r < n; ++r) {
    auto c = std::make_unique<cs_column>();
    c->rows = g.hdr[r].keys;
    c->nbytes = g.hdr[r].bytes;
    c->chars = dev_wrap(ptr<uint8_t>(g.chrs) + chr_piece * r, (size_t)g.hdr[r].bytes);
    c->offsets = dev_wrap(ptr<uint8_t>(g.offs) + off_piece * r, sizeof(int64_t) * (size_t)(g.hdr[r].keys + 1));
    const bool null_first = g.hdr[r].null_first && g.hdr[r].keys > 0;
    if (null_first) c->validity = null_first_mask(g.hdr[r].keys, s);
    c->null_count = null_first ? 1 : 0;
    g.cols.push_back(std::move(c));
  }
  return g;
}

// ---- the merge partitioned by key RANGE --------------------------------------------------------------------------------
// Splitters from a strided sample of every rank's sorted keys cut the key space into one range per rank; every local key
// goes to its range's owner (the local keys are sorted: contiguous slices; one all-to-all for the lengths, one for the
// bytes); the owner merges what it receives -- 1/G of the keys -- and returns every sender the positions of its keys in
// the merged range; an all-gather of the merged ranges, in rank order, is the global sorted key set (what
// NVCategory::create_from_categories makes of the gathered key sets, NVCategory.cu:430-514), and a local key's global
// code is its range's base plus the position that came back.
constexpr int64_t kPartitionMinKeys = (int64_t)1 << 21;
constexpr int kSplitterSamplesPerRank = 64;  // per destination rank

// cut[j + 1] = index of the first local key (from `first` on: a null key stays in range 0) that is not below splitter j
// (custring.inl:240-261: unsigned bytewise, shorter is less)
__global__ void k_range_cuts(ColView keys, int64_t first, ColView split, int nsplit, int64_t* __restrict__ cut) {
  const int j = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (j >= nsplit) return;
  const uint8_t* sp = split.chars + split.offsets[j];
  const int64_t sn = split.offsets[j + 1] - split.offsets[j];
  int64_t lo = first, hi = keys.rows;
  while (lo < hi) {
    const int64_t mid = lo + (hi - lo) / 2;
    const uint8_t* kp = keys.chars + keys.offsets[mid];
    const int64_t kn = keys.offsets[mid + 1] - keys.offsets[mid];
    const int64_t m = kn < sn ? kn : sn;
    int cmp = 0;
    for (int64_t i = 0; i < m && cmp == 0; ++i) cmp = (int)kp[i] - (int)sp[i];
    if (cmp == 0) cmp = kn < sn ? -1 : (kn > sn ? 1 : 0);
    if (cmp < 0) lo = mid + 1;
    else hi = mid;
  }
  cut[j + 1] = lo;
}
__global__ void k_key_lens(const int64_t* __restrict__ off, int64_t n, int32_t* __restrict__ lens) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) lens[i] = (int32_t)(off[i + 1] - off[i]);
}
// table[i] = base of key i's range + its position in the merged range (`cut`: nranks + 1 entries, `base`: nranks)
__global__ void k_range_table(const int32_t* __restrict__ back, const int64_t* __restrict__ cut, const int64_t* __restrict__ base, int nranks, int64_t n,
                              int32_t* __restrict__ table) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  int d = 0;
  while (d + 1 < nranks && i >= cut[d + 1]) ++d;
  table[i] = (int32_t)(base[d] + back[i]);
}
Buf upload_i64(const std::vector<int64_t>& v, hipStream_t s) {
  Buf b = dev_alloc(sizeof(int64_t) * std::max<size_t>(v.size(), 1), s);
  if (!v.empty()) CS_HIP(hipMemcpyAsync(b->p, v.data(), sizeof(int64_t) * v.size(), hipMemcpyHostToDevice, s));
  CS_HIP(hipStreamSynchronize(s));  // (pageable source)
  return b;
}
std::unique_ptr<cs_column> rows_at(const cs_column* col, const std::vector<int32_t>& pos, hipStream_t s) {
  Buf d = dev_alloc(sizeof(int32_t) * std::max<size_t>(pos.size(), 1), s);
  if (!pos.empty()) CS_HIP(hipMemcpyAsync(d->p, pos.data(), sizeof(int32_t) * pos.size(), hipMemcpyHostToDevice, s));
  CS_HIP(hipStreamSynchronize(s));
  return std::unique_ptr<cs_column>(gather_rows(col, ptr<const int32_t>(d), (int64_t)pos.size(), s));
}

// Failure agreement: between the collectives below sit multi-GB allocations and consistency checks that may
// throw on ONE rank (the owner of a skewed range running out of memory, say).  Every stretch of local work runs under
// `attempt`, which turns a throw into `failed`; the next exchange -- the header gather of sample_keys, the size exchange
// of exchange_range_sizes (one more slot per row) or the `agree` of make_room and merge_range, in front of an all-to-all
// whose sizes are already fixed -- carries the status, and all ranks stop there together.
// CS_DIST_TEST_FAIL_AT=<rank>:<stage> simulates a failure in stage 1..4 (tests).
struct PartitionedMerge {
  const Exchange& x;
  const cs_category* local;
  const std::vector<KeyHeader>& heads;  // the ranks' key sets (the first exchange): heads[r].null_first = rank r has the null key
  hipStream_t s = x.s;
  const int n = x.nranks;
  const cs_column* keys = local->keys.get();                               // this rank's sorted keys,
  const int64_t K = keys->rows, first = heads[x.rank].null_first ? 1 : 0;  // how many, and the first that is not the null key
  Failure failed;                 // this rank's failure since the last agreement; once set, `attempt` runs nothing more
  int stage = 0, fail_stage = 0;  // stages begun; the one CS_DIST_TEST_FAIL_AT names for this rank
  // (the buffers below stay to the end: the pool gets all of them back when the merge is over, the last made first)
  std::unique_ptr<cs_column> sample;  // sample_keys: this rank's strided sample (gathered from there)
  Gathered samples;                   // sample_keys -> cut_ranges: every rank's sample
  std::vector<int64_t> cut, byte_at;  // cut_ranges: keys cut[d] .. cut[d + 1] go to rank d; byte_at[d] = where key cut[d] starts in the chars
  Buf d_cut;                          // `cut` on the device: k_range_cuts writes it, k_range_table (remap_rows) reads it
  std::vector<int64_t> in_key_at, in_byte_at;  // exchange_range_sizes: sender r's keys / bytes stand at [r] .. [r + 1] of what arrives here
  Buf lens, in_lens, in_chars;  // make_room -> send_keys -> merge_range: the key lengths here; the lengths and bytes that arrive
  Buf back;                     // make_room -> return_positions -> remap_rows: per local key its position in its range
  std::vector<std::unique_ptr<cs_column>> parts;  // merge_range: the senders' slices as columns over in_chars
  std::unique_ptr<cs_category> range;             // merge_range -> return_positions: the category of the slices (none when nothing arrived)
  std::unique_ptr<cs_column> range_keys;          // merge_range -> gather_ranges: this rank's merged range

  cs_category* run() {
    if (const char* f = cs::cfg("CS_DIST_TEST_FAIL_AT")) {
      int r = -1, st = 0;
      if (sscanf(f, "%d:%d", &r, &st) == 2 && r == x.rank) fail_stage = st;
    }
    sample_keys();           // stage 1, then the samples to everybody
    cut_ranges();            // stage 2
    exchange_range_sizes();  // who sends how much to whom
    make_room();             // stage 3, agreed on
    send_keys();             // two all-to-alls: lengths, bytes
    merge_range();           // stage 4, agreed on
    return_positions();      // one all-to-all back
    return remap_rows(gather_ranges());
  }
  template <class F>
  void attempt(F&& work) {
    ++stage;
    if (failed.status) return;
    failed = caught([&] {
      if (stage == fail_stage) fail(CS_ERR_ALLOC, "simulated failure in stage " + std::to_string(stage) + " of the partitioned merge (CS_DIST_TEST_FAIL_AT)");
      work();
    });
  }
  // ---- stage 1: a strided sample of this rank's keys; every rank's sample on every rank
  void sample_keys() {
    attempt([&] {
      std::vector<int32_t> pos;
      const int64_t want = (int64_t)kSplitterSamplesPerRank * n, step = std::max<int64_t>((K - first) / want, 1);
      for (int64_t i = first; i < K; i += step) pos.push_back((int32_t)i);
      sample = rows_at(keys, pos, s);
    });
    samples = gather_columns(x, sample.get(), headers_or_own_failure(x, sample.get(), failed, "splitter samples"), "splitter samples");
  }
  // ---- stage 2: the samples pooled, sorted, cut into n ranges by n - 1 splitters (fewer when the pool is small: the last
  // ranges stay empty); this rank's keys by range
  void cut_ranges() {
    cut.assign(n + 1, K);
    byte_at.assign(n + 1, 0);
    cut[0] = 0;
    attempt([&] {
      std::unique_ptr<cs_column> splitters;
      int nsplit = 0;
      if (samples.total_keys > 0) {
        std::unique_ptr<cs_column> pooled(concat_columns(samples.ptrs(), s));
        std::unique_ptr<cs_category> pool(category_build(pooled.get(), s));  // sorted, unique: the same on every rank
        const int64_t M = pool->keys->rows, stride = std::max<int64_t>(M / n, 1);
        std::vector<int32_t> sp;
        for (int64_t i = stride; i < M && (int)sp.size() < n - 1; i += stride) sp.push_back((int32_t)i);
        nsplit = (int)sp.size();
        if (nsplit) splitters = rows_at(pool->keys.get(), sp, s);
      }
      d_cut = upload_i64(cut, s);
      if (nsplit && K > 0) {
        hipLaunchKernelGGL(k_range_cuts, dim3((unsigned)((nsplit + 255) / 256)), dim3(256), 0, s, view_of(keys), first, view_of(splitters.get()), nsplit, ptr<int64_t>(d_cut));
        CS_HIP(hipGetLastError());
        CS_HIP(hipMemcpyAsync(cut.data(), d_cut->p, sizeof(int64_t) * (n + 1), hipMemcpyDeviceToHost, s));
        CS_HIP(hipStreamSynchronize(s));
        for (int d = nsplit + 1; d <= n; ++d) cut[d] = K;
        for (int d = 1; d <= n; ++d) cut[d] = std::max(cut[d], cut[d - 1]);
        CS_HIP(hipMemcpyAsync(d_cut->p, cut.data(), sizeof(int64_t) * (n + 1), hipMemcpyHostToDevice, s));
        CS_HIP(hipStreamSynchronize(s));
      }
      if (K > 0) {
        for (int d = 0; d <= n; ++d) CS_HIP(hipMemcpyAsync(&byte_at[d], keys->d_offsets() + cut[d], sizeof(int64_t), hipMemcpyDeviceToHost, s));
        CS_HIP(hipStreamSynchronize(s));
      }
    });
  }
  // ---- every rank's (keys, bytes) per destination and its status, all-gathered: what arrives here, and from whom
  void exchange_range_sizes() {
    const size_t slots = 2 * (size_t)n + 1;
    std::vector<int64_t> mine(slots, 0);
    for (int d = 0; d < n && !failed.status; ++d) {
      mine[2 * d] = cut[d + 1] - cut[d];
      mine[2 * d + 1] = byte_at[d + 1] - byte_at[d];
    }
    mine[2 * n] = failed.status;
    const std::vector<int64_t> counts = exchange_records(x, mine, "the exchange of the range sizes failed");
    stop_if_failed(counts, slots, failed, "before the exchange of the range sizes", "", "range sizes");
    in_key_at.assign(n + 1, 0);
    in_byte_at.assign(n + 1, 0);
    for (int r = 0; r < n; ++r) {
      in_key_at[r + 1] = in_key_at[r] + counts[slots * r + 2 * x.rank];
      in_byte_at[r + 1] = in_byte_at[r] + counts[slots * r + 2 * x.rank + 1];
    }
  }
  // ---- stage 3: room for what arrives (the owner of a skewed range may not have it: agreed on BEFORE anything is sent)
  void make_room() {
    attempt([&] {
      lens = dev_alloc(sizeof(int32_t) * (size_t)std::max<int64_t>(K, 1), s);
      if (K) hipLaunchKernelGGL(k_key_lens, dim3((unsigned)((K + 255) / 256)), dim3(256), 0, s, keys->d_offsets(), K, ptr<int32_t>(lens));
      in_lens = dev_alloc(sizeof(int32_t) * (size_t)std::max<int64_t>(in_key_at[n], 1), s);
      in_chars = dev_alloc((size_t)in_byte_at[n] + 16, s);
      back = dev_alloc(sizeof(int32_t) * (size_t)std::max<int64_t>(K, 1), s);
    });
    agree(x, failed, "receive buffers of the key ranges");
  }
  // ---- the keys travel, every one to its range's owner: lengths, then bytes
  void send_keys() {
    exchange_slices(x, /*send=*/lens->p, /*send_at=*/cut, /*recv=*/in_lens->p, /*recv_at=*/in_key_at, sizeof(int32_t), "key lengths");
    const uint8_t* my_chars = keys->nbytes > 0 ? keys->d_chars() + byte_at[0] : ptr<const uint8_t>(in_chars);  // (a valid address when nothing is sent)
    exchange_slices(x, /*send=*/my_chars, /*send_at=*/byte_at, /*recv=*/in_chars->p, /*recv_at=*/in_byte_at, 1, "key bytes");
  }
  // ---- stage 4: this rank's range -- the parts that arrived (each sorted and unique), merged
  void merge_range() {
    attempt([&] {
      std::vector<const cs_column*> part_ptrs;
      for (int r = 0; r < n; ++r) {
        const int64_t got_keys = in_key_at[r + 1] - in_key_at[r], got_bytes = in_byte_at[r + 1] - in_byte_at[r];
        if (got_keys == 0) continue;
        Built b(got_keys, Nulls::none, s);  // (its chars are the received bytes, wrapped: no alloc_chars)
        std::unique_ptr<cs_column>& c = b.col;
        const int64_t total = b.scan(ptr<const int32_t>(in_lens) + in_key_at[r]);
        if (total != got_bytes) fail(CS_ERR_INTERNAL, "category_build_distributed: a received part's lengths do not add up to its bytes");
        c->chars = dev_wrap(ptr<uint8_t>(in_chars) + in_byte_at[r], (size_t)got_bytes);
        // (a null key travels as a key of no bytes at the head of its sender's slice for range 0 -- the sizes exchange said
        // which ranks have one)
        const bool null_first = x.rank == 0 && heads[r].null_first;
        if (null_first) c->validity = null_first_mask(got_keys, s);
        c->null_count = null_first ? 1 : 0;
        part_ptrs.push_back(c.get());
        parts.push_back(std::move(c));
      }
      if (!part_ptrs.empty()) {
        std::unique_ptr<cs_column> all(concat_columns(part_ptrs, s));
        range.reset(category_build(all.get(), s));
        range_keys = std::move(range->keys);
      } else {
        range_keys.reset(make_all_null(0, s));
      }
    });
    agree(x, failed, "merge of the received key range");
  }
  // ---- positions back to the senders (in the senders' key order: slice d lands at this rank's keys cut[d] ..)
  void return_positions() {
    const void* codes = range ? range->values->p : back->p;  // (a valid address when nothing arrived)
    exchange_slices(x, /*send=*/codes, /*send_at=*/in_key_at, /*recv=*/back->p, /*recv_at=*/cut, sizeof(int32_t), "merged positions");
  }
  // ---- the merged ranges to everybody: in rank order they are the global key set
  Gathered gather_ranges() { return gather_columns(x, range_keys.get(), gather_headers(x, range_keys.get(), 0, "merged ranges"), "merged ranges"); }
  // ---- a local key's global code is its range's base plus the position that came back; the rows' codes through that table
  cs_category* remap_rows(const Gathered& ranges) {
    std::vector<int64_t> base(n, 0);
    std::vector<const cs_column*> nonempty;
    int64_t run = 0;
    for (int r = 0; r < n; ++r) {
      base[r] = run;
      run += ranges.hdr[r].keys;
      if (ranges.hdr[r].keys > 0) nonempty.push_back(ranges.cols[r].get());
    }
    // (the same sum on every rank: all of them stop here together)
    if (run >= ((int64_t)1 << 31)) fail(CS_ERR_RANGE, "category_build_distributed: more than 2^31 keys in all");
    auto merged = std::make_unique<cs_category>();
    merged->rows = local->rows;
    merged->keys.reset(nonempty.empty() ? make_all_null(0, s) : concat_columns(nonempty, s));
    merged->values = dev_alloc(sizeof(int32_t) * (size_t)std::max<int64_t>(local->rows, 1), s);
    if (K > 0 && local->rows > 0) {
      Buf table = dev_alloc(sizeof(int32_t) * (size_t)K, s), d_base = upload_i64(base, s);
      hipLaunchKernelGGL(k_range_table, dim3((unsigned)((K + 255) / 256)), dim3(256), 0, s, ptr<const int32_t>(back), ptr<const int64_t>(d_cut), ptr<const int64_t>(d_base), n, K,
                         ptr<int32_t>(table));
      CS_HIP(hipGetLastError());
      remap_codes(ptr<const int32_t>(local->values), local->rows, ptr<const int32_t>(table), ptr<int32_t>(merged->values), s);
    }
    CS_HIP(hipStreamSynchronize(s));  // (the gathered buffers leave scope; what follows the last collective fails locally, nobody waits)
    return merged.release();
  }
};

// the all-gather route: every rank merges the same key sets
cs_category* merge_gathered(const Exchange& x, const cs_category* local, std::vector<KeyHeader> heads) {
  const Gathered g = gather_columns(x, local->keys.get(), std::move(heads), "key sets");
  return merge_key_sets(local, g.ptrs(), x.rank, nullptr, x.s);  // (waits: the gathered buffers leave scope)
}

void build_distributed(const cs_column* col, const Exchange& x, bool run_alone, cs_category** out) {
  // the local build may fail (memory, a key too long): this rank then still takes part in the first exchange and tells
  // the others, so that nobody is left waiting in a collective
  std::unique_ptr<cs_category> local;
  Failure failed = caught([&] { local.reset(category_build(col, x.s)); });
  if (const char* f = cs::cfg("CS_DIST_TEST_FAIL"))  // tests: this rank's local build "fails"
    if (failed.status == 0 && atoi(f) == x.rank) {
      failed = {CS_ERR_ALLOC, "simulated failure of the local build (CS_DIST_TEST_FAIL)"};
      local.reset();
    }
  if (x.nranks == 1 && !run_alone) {  // the local codes are the global ones
    if (failed.status) fail(failed.status, failed.why);
    *out = local.release();
    return;
  }
  // (this rank's own failure is the one to report here)
  const std::vector<KeyHeader> heads = headers_or_own_failure(x, failed.status ? nullptr : local->keys.get(), failed, "key sets");
  int64_t total = 0;
  for (const KeyHeader& h : heads) total += h.keys;
  const char* force = cs::cfg("CS_DIST_PARTITIONED");  // tests: 1 = always (given an all-to-all), 0 = never
  const bool partitioned = x.alltoallv && x.nranks > 1 && (force ? atoi(force) != 0 : total >= kPartitionMinKeys);
  *out = partitioned ? PartitionedMerge{x, local.get(), heads}.run() : merge_gathered(x, local.get(), heads);
}

}  // namespace

extern "C" {

int cs_category_build_distributed_with(const cs_column* col, cs_allgather_fn allgather, void* ctx, int nranks, int rank, cs_stream stream,
                                       cs_category** out) {
  return cs_category_build_distributed_with2(col, allgather, nullptr, ctx, nranks, rank, stream, out);
}

int cs_category_build_distributed_with2(const cs_column* col, cs_allgather_fn allgather, cs_alltoallv_fn alltoallv, void* ctx, int nranks, int rank,
                                        cs_stream stream, cs_category** out) {
  return guard([&] {
    if (!col || !out || !allgather || nranks < 1 || rank < 0 || rank >= nranks) fail(CS_ERR_INVALID_ARG, "category_build_distributed: bad arguments");
    require_device();
    const Exchange x{allgather, alltoallv, ctx, nranks, rank, S(stream)};
    build_distributed(col, x, ctx != nullptr, out);  // (with a context the exchange runs even for one rank: a rank with itself)
  });
}

int cs_category_build_distributed(const cs_column* col, void* nccl_comm, int nranks, int rank, cs_stream stream, cs_category** out) {
  return guard([&] {
    if (!nccl_comm && nranks > 1) fail(CS_ERR_INVALID_ARG, "category_build_distributed: no communicator");
    if (nranks > 1 || nccl_comm) {
      resolve_rccl();
      if (!g_allgather) fail(CS_ERR_INTERNAL, "category_build_distributed: no RCCL in this process (ncclAllGather not found, librccl.so not loadable)");
    }
    const bool p2p = g_send && g_recv && g_group_start && g_group_end;
    const int rc = cs_category_build_distributed_with2(col, &rccl_allgather, p2p ? &rccl_alltoallv : nullptr, nccl_comm, nranks, rank, stream, out);
    if (rc != 0) fail(rc, cs_last_error());
  });
}

}  // extern "C"
