// Device-side greedy infill grammar: the per-token host loop of
// generation.py:528-687 (grammar flags -> sampling mask -> argmax -> commit
// -> next prefix) as one kernel appended to the captured decode step, so a
// batch of requests decodes for many steps without a host round trip.
//
// Per request r the step's logits row is `logits[(2r+1) * ldl]` (the last
// fed token of the request's two step slots, decode.py).  The kernel
//   1. derives the grammar state code from the request's flags
//      (_Span.spec, generation.py:549-630) -> keep[state][V] mask table,
//   2. takes argmax over where(keep, logit, -100) (first index on ties, as
//      np.argmax over the reference's float64 softmax of the same masked
//      row: exp / normalise is monotone),
//   3. commits the id (_Span.commit, generation.py:632-687): flag updates,
//      control -> [id, eos], span end on eos / 100 tokens, next mask index,
//   4. writes the next step's feed (ids + meta rows 2r, 2r+1) and appends
//      the id to out_tok[r].
// One wave per request (latency-bound: a few dependent loads per request,
// all requests in parallel).  The number of requests still live after the
// step is counted into *alive, which the kernel's caller zeroes first
// (smer_grammar_greedy_step issues the memset on the same stream).
#include <type_traits>

#include "common.h"

namespace {
constexpr int ST_POS = 0, ST_FLAGS = 1, ST_LEN = 2, ST_MIDX = 3, ST_NMASK = 4, ST_DONE = 5,
              ST_NOWHOLE = 6, ST_COUNT = 7, ST_ERR = 8;
constexpr int F_SEP = 1, F_CONT = 2, F_PITCH = 4, F_REST = 8;
// token class bits (host builds cls[V] from the vocab)
constexpr int C_CONT = 1, C_PITCH = 2, C_DUR = 4, C_SEPSTR = 8, C_RESTSTR = 16, C_CTRL = 32;
}  // namespace

__device__ __forceinline__ int grammar_state(int flags, int len, int target, int no_whole) {
  if (flags & F_SEP) return 0;
  if (flags & F_CONT) return 1;
  if (flags & F_PITCH) return 2 + no_whole;
  if (flags & F_REST) return 4 + no_whole;
  if (len == 1) return target == 0 ? 10 : 5 + target;  // 'r' -> 10; d,o,p,t -> 6..9
  return 11 + no_whole;
}

// Commit id `idx` of request r (_Span.commit, generation.py:632-687): flag
// updates, control -> [id, eos], span end on eos / max_span tokens, next
// mask index; writes the next step's feed (rows 2r, 2r+1) and appends the
// id to out_tok[r] (bit 16: the redraw loop gave up on this draw).
// Returns whether the request is still live.  Lane 0 only.
__device__ bool grammar_commit(int r, int idx, bool fail, int flags, int len, int midx, int nmask, int cnt,
                               int pos, int32_t* st, const uint8_t* cls, int eos, int m0, int trash_pos,
                               int max_span, const int32_t* src_len, int64_t* ids, int32_t* meta, int M,
                               int32_t* out_tok, int cap) {
  const int c = cls[idx];
  int f = flags;
  if (c & C_CONT) f = (f | F_CONT) & ~F_SEP;
  if (c & C_PITCH) f = (f | F_PITCH) & ~(F_SEP | F_CONT);
  if (c & C_DUR) f &= ~(F_REST | F_PITCH);
  if (c & C_SEPSTR) f |= F_SEP;
  if (c & C_RESTSTR) f |= F_REST;
  if (cnt < cap) out_tok[(long)r * cap + cnt] = idx | (fail ? 0x10000 : 0);
  st[ST_COUNT] = cnt + 1;
  int feed[2], nf;
  bool end;
  if (c & C_CTRL) {  // this_in += [idx, eos]: the span ends
    end = true; feed[0] = idx; feed[1] = m0; nf = 2;
  } else if (idx == eos || len + 1 >= max_span) {  // last token dropped, m_0 takes its place
    end = true; feed[0] = m0; nf = 1;
  } else {
    end = false; feed[0] = idx; nf = 1;
  }
  bool done = false;
  int nlen = len + 1, nmidx = midx;
  if (end) {
    nmidx = midx + 1;
    if (nmidx >= nmask) {
      done = true;
      nf = 0;  // nothing more to feed
    } else {
      f = 0;
      nlen = 1;
    }
  }
  st[ST_MIDX] = nmidx;
  st[ST_LEN] = nlen;
  st[ST_FLAGS] = f;
  if (!done && pos + nf > trash_pos) {  // decoder prefix would overrun the cache
    st[ST_ERR] |= 1;
    done = true;
  }
  // next step's rows 2r (first) and 2r+1 (last): dummies unless fed
  const int skv = max(src_len[r], 1);
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int row = 2 * r + k;
    const int j = k - (2 - nf);  // index into feed for this row (row 2r+1 carries the last)
    const bool real = !done && j >= 0;
    ids[row] = real ? feed[j] : 0;
    meta[row] = real ? pos + j : trash_pos;
    meta[M + row] = r;
    meta[2 * M + row] = real ? pos + j + 1 : 1;
    meta[3 * M + row] = real ? skv : 1;
  }
  if (done) st[ST_DONE] = 1;
  else st[ST_POS] = pos + nf;
  return !done;
}

// RING: no memset / host copy per step.  ctl = {live count, tickets, step}
// (device, zeroed once by the caller); every request's block takes a ticket
// after adding itself to the live count, and the step's last block publishes
// the count to ring[step % ring_n] (host-visible pinned memory) and resets
// ctl for the next step.  The host reads the slot after the step's event.
__device__ __forceinline__ void grammar_ring_ticket(int32_t* ctl, int32_t* ring, int ring_n, int R) {
  const int t = __hip_atomic_fetch_add(&ctl[1], 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
  if (t == R - 1) {
    const int a = __hip_atomic_load(&ctl[0], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);
    const int s = __hip_atomic_load(&ctl[2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(&ring[s % ring_n], a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(&ctl[0], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(&ctl[1], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(&ctl[2], s + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

template <bool RING>
__global__ __launch_bounds__(64) void grammar_greedy_kernel(
    int R, int V, const float* __restrict__ logits, long ldl, int32_t* __restrict__ state,
    int nst, const int8_t* __restrict__ targets, int max_masks, const uint8_t* __restrict__ keep,
    const uint8_t* __restrict__ cls, int eos, int m0, int trash_pos, int max_span,
    const int32_t* __restrict__ src_len, int64_t* __restrict__ ids, int32_t* __restrict__ meta,
    int M, int32_t* __restrict__ out_tok, int cap, int32_t* __restrict__ alive,
    int32_t* __restrict__ ring, int ring_n) {
  // one wave per request; the whole state vector is read in one load
  // (lane k <- st[k]) alongside the logits row, then broadcast
  const int r = blockIdx.x, lane = threadIdx.x;
  int32_t* st = state + (long)r * nst;
  const int sv = lane < nst ? st[lane] : 0;
  const float* lr = logits + (long)(2 * r + 1) * ldl;
  float lg[5];
#pragma unroll
  for (int u = 0; u < 5; ++u) {
    const int i = lane + 64 * u;
    lg[u] = i < V ? lr[i] : -INFINITY;
  }
  const int done0 = __shfl(sv, ST_DONE, 64);
  if (done0) {  // wave-uniform
    if (RING && lane == 0) grammar_ring_ticket(alive, ring, ring_n, R);
    return;
  }
  const int flags = __shfl(sv, ST_FLAGS, 64), len = __shfl(sv, ST_LEN, 64),
            midx = __shfl(sv, ST_MIDX, 64), nmask = __shfl(sv, ST_NMASK, 64),
            nowhole = __shfl(sv, ST_NOWHOLE, 64), cnt = __shfl(sv, ST_COUNT, 64),
            pos = __shfl(sv, ST_POS, 64);
  const int code = grammar_state(flags, len, targets[(long)r * max_masks + midx], nowhole);
  const uint8_t* kp = keep + (long)code * V;
  float best = -INFINITY;
  int bi = 0x7fffffff;
  for (int u = 0; u < (V + 63) / 64 && u < 5; ++u) {
    const int i = lane + 64 * u;
    if (i < V) {
      const float x = kp[i] ? lg[u] : -100.f;
      if (x > best || bi == 0x7fffffff) { best = x; bi = i; }  // ascending i: first max kept
    }
  }
  for (int i = lane + 320; i < V; i += 64) {  // V > 320 (not the SMER vocab)
    const float x = kp[i] ? lr[i] : -100.f;
    if (x > best || bi == 0x7fffffff) { best = x; bi = i; }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ob = __shfl_xor(best, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; }
  }
  if (lane != 0) return;
  const bool l = grammar_commit(r, bi, false, flags, len, midx, nmask, cnt, pos, st, cls, eos, m0,
                                trash_pos, max_span, src_len, ids, meta, M, out_tok, cap);
  if (l) {
    if (RING) __hip_atomic_fetch_add(&alive[0], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else atomicAdd(alive, 1);  // integer count: order-independent
  }
  if (RING) grammar_ring_ticket(alive, ring, ring_n, R);
}

extern "C" int smer_grammar_greedy_step(int R, int V, const float* logits, long ldl,
                                        int32_t* state, int nst, const int8_t* targets,
                                        int max_masks, const uint8_t* keep, const uint8_t* cls,
                                        int eos, int m0, int trash_pos, int max_span,
                                        const int32_t* src_len, int64_t* ids, int32_t* meta,
                                        int32_t* out_tok, int cap, int32_t* alive,
                                        smer_stream_t stream) {
  SMER_REQUIRE(R > 0 && V > 0 && nst >= 9 && max_masks > 0 && cap > 0, "smer_grammar_greedy_step: sizes");
  SMER_REQUIRE(ldl >= V, "smer_grammar_greedy_step: logits row stride");
  SMER_REQUIRE(logits && state && targets && keep && cls && src_len && ids && meta && out_tok && alive,
               "smer_grammar_greedy_step: null pointer");
  SMER_REQUIRE(eos >= 0 && eos < V && m0 >= 0 && m0 < V && trash_pos > 0 && max_span > 1,
               "smer_grammar_greedy_step: token ids");
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(alive, 0, sizeof(int32_t), s) != hipSuccess)
    return smer_set_error(SMER_ERR_HIP, "smer_grammar_greedy_step: memset");
  hipLaunchKernelGGL(grammar_greedy_kernel<false>, dim3(R), dim3(64), 0, s, R, V,
                     logits, ldl, state, nst, targets, max_masks, keep, cls, eos, m0, trash_pos,
                     max_span, src_len, ids, meta, 2 * R, out_tok, cap, alive, nullptr, 0);
  SMER_CHECK_LAUNCH("smer_grammar_greedy_step");
  return SMER_OK;
}

extern "C" int smer_grammar_greedy_step_ring(int R, int V, const float* logits, long ldl,
                                             int32_t* state, int nst, const int8_t* targets,
                                             int max_masks, const uint8_t* keep, const uint8_t* cls,
                                             int eos, int m0, int trash_pos, int max_span,
                                             const int32_t* src_len, int64_t* ids, int32_t* meta,
                                             int32_t* out_tok, int cap, int32_t* ctl,
                                             int32_t* ring, int ring_n, smer_stream_t stream) {
  SMER_REQUIRE(R > 0 && V > 0 && nst >= 9 && max_masks > 0 && cap > 0 && ring_n > 0,
               "smer_grammar_greedy_step_ring: sizes");
  SMER_REQUIRE(ldl >= V, "smer_grammar_greedy_step_ring: logits row stride");
  SMER_REQUIRE(logits && state && targets && keep && cls && src_len && ids && meta && out_tok && ctl && ring,
               "smer_grammar_greedy_step_ring: null pointer");
  SMER_REQUIRE(eos >= 0 && eos < V && m0 >= 0 && m0 < V && trash_pos > 0 && max_span > 1,
               "smer_grammar_greedy_step_ring: token ids");
  // the ring is pinned host memory: its device-side address
  void* dring = nullptr;
  if (hipHostGetDevicePointer(&dring, ring, 0) != hipSuccess || dring == nullptr) {
    (void)hipGetLastError();
    dring = ring;
  }
  hipLaunchKernelGGL(grammar_greedy_kernel<true>, dim3(R), dim3(64), 0, (hipStream_t)stream, R, V,
                     logits, ldl, state, nst, targets, max_masks, keep, cls, eos, m0, trash_pos,
                     max_span, src_len, ids, meta, 2 * R, out_tok, cap, ctl, (int32_t*)dring, ring_n);
  SMER_CHECK_LAUNCH("smer_grammar_greedy_step_ring");
  return SMER_OK;
}

// ---------------------------------------------------------------------------
// Device-side sampled infill grammar (the plugin's default path,
// generation.py:33-95 + 528-687): the reference's float64 softmax of the
// masked logits, `weighted_sampling`'s normalisation and descending sort,
// `np.random.choice`'s cdf / searchsorted, and the redraw loop, consuming the
// numpy legacy MT19937 stream (`random_sample`: two 32-bit outputs per
// uniform) handed over from np.random.get_state() and back by the caller.
// One block (one wave) walks the requests in order, as the host loop draws
// them.  Arithmetic order (host equivalents):
//   S = np.sum(e): numpy's pairwise summation (8 accumulators, blocks of 128,
//       tests/test_sampling.py pins the replica against numpy itself);
//   T = np.add.accumulate(p)[-1], cdf = np.cumsum(p_sorted): sequential;
//   u = (a >> 5, b >> 6) -> (a * 2^26 + b) / 2^53, idx = first cdf > u.
// exp is the device's float64 exp (within 1 ulp of numpy's; a draw could
// differ only if u fell within that distance of a cdf step), and exact ties
// between probabilities sort by descending index, the order a stable argsort
// reversed gives (numpy's introsort order for equal float32 logits is
// implementation-defined): documented in DESIGN.md.
// ---------------------------------------------------------------------------
namespace {
constexpr int SMX = 512;  // vocabulary slots of the sort (V <= 512)

__device__ __forceinline__ uint32_t mt_temper(uint32_t y) {
  y ^= y >> 11;
  y ^= (y << 7) & 0x9d2c5680u;
  y ^= (y << 15) & 0xefc60000u;
  y ^= y >> 18;
  return y;
}
// numpy's mt19937_gen over the LDS key, by the whole wave: each range's
// reads all happen before its writes (the sequential loop reads key[i + 1]
// before rewriting it), ranges in the order whose inputs they need
__device__ void mt_twist(uint32_t* key, int lane) {
  auto mix = [](uint32_t ki, uint32_t ki1, uint32_t km) {
    const uint32_t y = (ki & 0x80000000u) | (ki1 & 0x7fffffffu);
    return km ^ (y >> 1) ^ ((0u - (y & 1u)) & 0x9908b0dfu);
  };
  const int lo[3] = {0, 227, 454}, hi[3] = {227, 454, 623};
  const int off[3] = {397, -227, -227};
  for (int ph = 0; ph < 3; ++ph) {
    uint32_t nv[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int i = lo[ph] + lane + 64 * u;
      nv[u] = i < hi[ph] ? mix(key[i], key[i + 1], key[i + off[ph]]) : 0u;
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int i = lo[ph] + lane + 64 * u;
      if (i < hi[ph]) key[i] = nv[u];
    }
    __syncthreads();
  }
  uint32_t last = mix(key[623], key[0], key[396]);
  __syncthreads();
  if (lane == 0) key[623] = last;
  __syncthreads();
}
__device__ __forceinline__ uint32_t mt_next(uint32_t* key, int& pos, int lane) {
  if (pos >= 624) {  // wave-uniform
    mt_twist(key, lane);
    pos = 0;
  }
  return mt_temper(key[pos++]);
}
// numpy legacy random_sample
__device__ __forceinline__ double mt_uniform(uint32_t* key, int& pos, int lane) {
  const int32_t a = (int32_t)(mt_next(key, pos, lane) >> 5);
  const int32_t b = (int32_t)(mt_next(key, pos, lane) >> 6);
  return (a * 67108864.0 + b) / 9007199254740992.0;
}
// numpy's pairwise_sum (loops_utils.h.src) for one contiguous block
__device__ double np_pairwise_leaf(const double* a, int n) {
  if (n < 8) {
    double r = 0.;
    for (int i = 0; i < n; ++i) r += a[i];
    return r;
  }
  double r[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) r[j] = a[j];
  int i = 8;
  for (; i < n - (n % 8); i += 8) {
    double x[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) x[j] = a[i + j];
#pragma unroll
    for (int j = 0; j < 8; ++j) r[j] += x[j];
  }
  double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
  for (; i < n; ++i) res += a[i];
  return res;
}
template <int DEPTH>
__device__ double np_pairwise(const double* a, int n) {
  if constexpr (DEPTH == 0) {
    return np_pairwise_leaf(a, n);
  } else {
    if (n <= 128) return np_pairwise_leaf(a, n);
    int n2 = n / 2;
    n2 -= n2 % 8;
    return np_pairwise<DEPTH - 1>(a, n2) + np_pairwise<DEPTH - 1>(a + n2, n - n2);
  }
}
// sequential left-to-right sum of a[0..n) from 0 (np.add.accumulate's last
// element, builtin sum()); LDS loads issued 8 at a time ahead of their adds
__device__ double seq_sum(const double* a, int n) {
  double t = 0.;
  int i = 0;
  for (; i + 8 <= n; i += 8) {
    double x[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) x[j] = a[i + j];
#pragma unroll
    for (int j = 0; j < 8; ++j) t += x[j];
  }
  for (; i < n; ++i) t += a[i];
  return t;
}
// c[i] = a[0] + ... + a[i], sequential (np.cumsum); returns c[n - 1].  A
// batch's 8 sums are formed before its 8 stores (a store right behind each
// add stalled on it: 25.7 vs 13.6 cycles per element for the plain sum)
__device__ double seq_cumsum(const double* a, double* c, int n) {
  double t = 0.;
  int i = 0;
  for (; i + 8 <= n; i += 8) {
    double x[8], r[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) x[j] = a[i + j];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      t += x[j];
      r[j] = t;
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int j = 0; j < 8; ++j) c[i + j] = r[j];
  }
  for (; i < n; ++i) {
    t += a[i];
    c[i] = t;
  }
  return t;
}
// value of lane ^ X (X a power of two < 64): DPP for 1 and 2, swizzle
// (no LDS traffic) within 32-lane halves for 4-16, the half swap for 32
template <int X>
__device__ __forceinline__ uint32_t lane_xor(uint32_t v) {
  if constexpr (X == 1) return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0xB1, 0xF, 0xF, false);
  else if constexpr (X == 2) return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x4E, 0xF, 0xF, false);
  else if constexpr (X < 32) return (uint32_t)__builtin_amdgcn_ds_swizzle((int)v, (X << 10) | 0x1F);
  else {
    const auto r = __builtin_amdgcn_permlane32_swap(v, v, false, false);
    return (__lane_id() < 32) ? r[1] : r[0];
  }
}
template <int X>
__device__ __forceinline__ uint64_t lane_xor64(uint64_t v) {
  return ((uint64_t)lane_xor<X>((uint32_t)(v >> 32)) << 32) | lane_xor<X>((uint32_t)v);
}

// bitonic sort, descending, of 64 E keys held E per lane (element s = lane
// * E + e): partners at distance >= E sit in lane ^ (dist / E), nearer ones
// in the same lane
template <int E>
__device__ __forceinline__ void sort_desc(uint64_t (&kv)[E], int lane) {
#pragma unroll
  for (int k = 2; k <= 64 * E; k <<= 1) {
#pragma unroll
    for (int jj = k >> 1; jj > 0; jj >>= 1) {
      if (jj >= E) {
        const int lx = jj / E;
        const bool lower = (lane & lx) == 0;
#pragma unroll
        for (int j = 0; j < E; ++j) {
          const int e = lane * E + j;
          const bool desc = (e & k) == 0;
          uint64_t o;
          switch (lx) {
            case 1: o = lane_xor64<1>(kv[j]); break;
            case 2: o = lane_xor64<2>(kv[j]); break;
            case 4: o = lane_xor64<4>(kv[j]); break;
            case 8: o = lane_xor64<8>(kv[j]); break;
            case 16: o = lane_xor64<16>(kv[j]); break;
            default: o = lane_xor64<32>(kv[j]); break;
          }
          const uint64_t mx = kv[j] > o ? kv[j] : o, mn = kv[j] > o ? o : kv[j];
          kv[j] = (lower == desc) ? mx : mn;
        }
      } else {
#pragma unroll
        for (int j = 0; j < E; ++j) {
          if (j & jj) continue;
          const int e = lane * E + j;
          const bool desc = (e & k) == 0;
          const uint64_t a0 = kv[j], a1 = kv[j | jj];
          const bool sw = desc ? a1 > a0 : a0 > a1;
          kv[j] = sw ? a1 : a0;
          kv[j | jj] = sw ? a0 : a1;
        }
      }
    }
  }
}

// fast path of the sampler: sort the first 64 E compacted keys (E per lane)
// and gather the p of sort positions < NA into sp
template <int E>
__device__ __forceinline__ void fast_sort_gather(const uint64_t* kA, int lane, int NA, int (&sidx)[8], double* sp,
                                                 const double* pe) {
  uint64_t k[E];
#pragma unroll
  for (int e = 0; e < E; ++e) k[e] = kA[lane * E + e];
  sort_desc<E>(k, lane);
#pragma unroll
  for (int e = 0; e < E; ++e) {
    const int s = lane * E + e;
    sidx[e] = (int)(uint32_t)k[e];
    if (s < NA) sp[s] = pe[sidx[e]];
  }
}

// np.sum's pairwise order over a[0..n) with the leaves' eight accumulator
// chains summed by separate lanes: lane 8L + j runs chain j of leaf L (the
// leaves are the blocks of <= 128 the recursion stops at, in order), lane 0
// then adds each leaf's tree and remainder and the leaves in the recursion's
// order -- the same additions in the same order as numpy's one thread
// leaf blocks of numpy's pairwise recursion over [a0, a0 + n) into lv
// (start, length pairs; lv[16] = count)
template <int DEPTH>
__device__ void pw_split(int* lv, int a0, int n) {
  if (DEPTH == 0 || n <= 128) {
    const int q = lv[16];
    lv[2 * q] = a0;
    lv[2 * q + 1] = n;
    lv[16] = q + 1;
    return;
  }
  if constexpr (DEPTH > 0) {
    int n2 = n / 2;
    n2 -= n2 % 8;
    pw_split<DEPTH - 1>(lv, a0, n2);
    pw_split<DEPTH - 1>(lv, a0 + n2, n - n2);
  }
}
template <int DEPTH>
__device__ double pw_combine(const double* leafsum, int& li, int n) {
  if (DEPTH == 0 || n <= 128) return leafsum[li++];
  if constexpr (DEPTH > 0) {
    int n2 = n / 2;
    n2 -= n2 % 8;
    const double x = pw_combine<DEPTH - 1>(leafsum, li, n2);
    return x + pw_combine<DEPTH - 1>(leafsum, li, n - n2);
  }
  return 0.;
}
// all 64 lanes call; scratch: 72 doubles of LDS, lv: 17 ints of LDS
__device__ double np_pairwise_par(const double* a, int n, double* scratch, int* lv, int lane) {
  if (lane == 0) {
    lv[16] = 0;
    pw_split<3>(lv, 0, n);
  }
  __syncthreads();
  const int nl = lv[16];
  const int leaf = lane >> 3, j = lane & 7;
  double r = 0.;
  if (leaf < nl && lv[2 * leaf + 1] >= 8) {
    const double* b = a + lv[2 * leaf];
    const int len = lv[2 * leaf + 1];
    const int m = len - len % 8;
    r = b[j];
    for (int i = 8; i < m; i += 8) r += b[i + j];
  }
  scratch[lane] = r;
  __syncthreads();
  double res = 0.;
  if (lane == 0) {
    for (int q = 0; q < nl; ++q) {
      const double* b = a + lv[2 * q];
      const int len = lv[2 * q + 1];
      double t;
      int i;
      if (len < 8) {
        t = 0.;
        i = 0;
      } else {
        const double* rr = scratch + 8 * q;
        t = ((rr[0] + rr[1]) + (rr[2] + rr[3])) + ((rr[4] + rr[5]) + (rr[6] + rr[7]));
        i = len - len % 8;
      }
      for (; i < len; ++i) t += b[i];
      scratch[64 + q] = t;
    }
    int li = 0;
    res = pw_combine<3>(scratch + 64, li, n);
  }
  __syncthreads();
  return res;
}

// sort position: larger probability first; equal probabilities by
// descending index
__device__ __forceinline__ bool before(double pa, int ia, double pb, int ib) {
  return pa > pb || (pa == pb && ia > ib);
}
}  // namespace

// order-preserving uint32 image of a float (larger float, larger image)
__device__ __forceinline__ uint32_t f32_ord(float f) {
  const uint32_t u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

#ifndef SMER_SAMPLE_STAMPS
#define SMER_SAMPLE_STAMPS 0  // tools/build_variant.sh ... -DSMER_SAMPLE_STAMPS=1: phase clocks in mt[640..]
#endif
#define SSTAMP(k) do { if (SMER_SAMPLE_STAMPS && !ROWS && lane == 0) mt[640 + (k)] = (uint32_t)__builtin_amdgcn_s_memtime(); } while (0)

// TP: the request's temperature and nucleus threshold come from tp[r] (double
// [R, 2]: t, p; p < 0 = None), read from device memory on every step, so a
// captured step serves any values.  e = exp(masked / t) (mask first, then a
// true float64 division, generation.py:28-30 of the reference); with p >= 0
// the reference's `nucleus` (generation.py:11-25) replaces weighted_sampling:
//   q = probs / (T + 1e-5), sorted descending, c = cumsum(q_sorted),
//   candidates = sort positions 0 .. first(c > p) (all when none exceeds p),
//   cp = q / sum(q[candidates]), cdf = cumsum(cp) / cdf[-1], one uniform.
// sum(q[candidates]) is c at the last candidate: builtin sum() from 0 and
// np.cumsum add the same numbers in the same order.  !TP is t = 1, p = None
// with the division folded away (x / 1.0 is exact: the same bits).
// ROWS: one MT19937 stream per request (mt + r * ldmt: 624 key words and the
// position) instead of the one shared stream, so nothing orders the draws
// across requests: one block per request (r = blockIdx.x) runs the same body
// on its own stream, and the live count is taken as grammar_greedy_kernel
// takes it (atomic add, then the ticket).  !ROWS is the serial walk over
// the shared stream, whose draw order is the host loop's.
template <bool RING, bool TP, bool ROWS>
__global__ __launch_bounds__(64) void grammar_sample_kernel(
    int R, int V, const float* __restrict__ logits, long ldl, int32_t* __restrict__ state, int nst,
    const int8_t* __restrict__ targets, int max_masks, const uint8_t* __restrict__ keep,
    const uint8_t* __restrict__ reject, const uint8_t* __restrict__ cls, int eos, int m0, int trash_pos,
    int max_span, const int32_t* __restrict__ src_len, int64_t* __restrict__ ids,
    int32_t* __restrict__ meta, int M, int32_t* __restrict__ out_tok, int cap,
    int32_t* __restrict__ alive, int32_t* __restrict__ ring, int ring_n, uint32_t* __restrict__ mt,
    const double* __restrict__ tp, long ldmt) {
  // one wave; element i of a row lives in lane i / 8, slot i % 8
  __shared__ uint32_t key[624];
  __shared__ double pe[SMX];   // e, then p by vocabulary index
  __shared__ double sp[SMX];   // p in sort order, then the normalised cdf
  __shared__ double cq[TP ? SMX : 1];  // nucleus: c, the cumulative sum of the sorted q
  __shared__ uint64_t kA[SMX];  // fast path: the compacted keys of set A
  __shared__ double bc[2];
  __shared__ int pwl[17];
  __shared__ __attribute__((aligned(16))) uint8_t tk[13 * SMX], tr[13 * SMX];  // keep / reject tables
  __shared__ uint8_t tcls[SMX];
  const int lane = threadIdx.x;
  const int r_lo = ROWS ? (int)blockIdx.x : 0, r_hi = ROWS ? r_lo + 1 : R;
  if constexpr (ROWS) mt += (long)r_lo * ldmt;
  SSTAMP(0);
  // every input load of the step in one batch (one memory latency, not a
  // chain of them): the MT key, the grammar tables, the first request
  {
    uint32_t kw[10];
#pragma unroll
    for (int u = 0; u < 10; ++u) kw[u] = lane + 64 * u < 624 ? mt[lane + 64 * u] : 0u;
    // the tables as 4-B words where whole (any 4-B alignment of the bases
    // is the caller's: torch allocations are), the tail bytes one by one
    const int nt = 13 * V, nw = ((((uintptr_t)keep | (uintptr_t)reject) & 3) == 0) ? nt / 4 : 0;
    constexpr int WPL = 13 * SMX / 4 / 64;  // words per lane
    uint32_t bk[WPL], br[WPL];
#pragma unroll
    for (int u = 0; u < WPL; ++u) {
      const int w = lane + 64 * u;
      bk[u] = w < nw ? reinterpret_cast<const uint32_t*>(keep)[w] : 0u;
      br[u] = w < nw ? reinterpret_cast<const uint32_t*>(reject)[w] : 0u;
    }
#pragma unroll
    for (int u = 0; u < 10; ++u)
      if (lane + 64 * u < 624) key[lane + 64 * u] = kw[u];
#pragma unroll
    for (int u = 0; u < WPL; ++u) {
      reinterpret_cast<uint32_t*>(tk)[lane + 64 * u] = bk[u];
      reinterpret_cast<uint32_t*>(tr)[lane + 64 * u] = br[u];
    }
    for (int i = 4 * nw + lane; i < nt; i += 64) {
      tk[i] = keep[i];
      tr[i] = reject[i];
    }
    for (int i = lane; i < V; i += 64) tcls[i] = cls[i];
  }
  // a request's state row, mask targets and logits (indices clamped, not
  // guarded: a guarded load waits right behind itself); request 0's with the
  // batch above, request r + 1's under request r's work
  auto fetch = [&](int r, int& sv, int& tgv, float (&lg)[8], double& tpv) {
    const int rr = min(r, R - 1);
    if constexpr (TP) tpv = tp[2 * (long)rr + (lane & 1)];  // even lanes t, odd lanes p
    sv = state[(long)rr * nst + min(lane, nst - 1)];
    tgv = (int)targets[(long)rr * max_masks + min(lane, max_masks - 1)];
    const float* lr = logits + (long)(2 * rr + 1) * ldl;
#pragma unroll
    for (int j = 0; j < 8; ++j) lg[j] = lr[min(lane * 8 + j, V - 1)];
  };
  int sv_n, tgv_n;
  float lg_n[8];
  double tp_n = 0.;
  fetch(r_lo, sv_n, tgv_n, lg_n, tp_n);
  int pos = (int)mt[624];
  __syncthreads();
  SSTAMP(1);
  int live = 0;
  for (int r = r_lo; r < r_hi; ++r) {
    int32_t* st = state + (long)r * nst;
    const int sv = sv_n, tgv = tgv_n;
    float lg8[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) lg8[j] = lg_n[j];
    const double tpv = tp_n;
    if constexpr (!ROWS) fetch(r + 1, sv_n, tgv_n, lg_n, tp_n);
    if (__shfl(sv, ST_DONE, 64)) {  // wave-uniform
      if constexpr (ROWS) {  // its stream stays as it is; the step still counts the block
        if (RING && lane == 0) grammar_ring_ticket(alive, ring, ring_n, R);
        return;
      }
      continue;
    }
    const double temp = TP ? __shfl(tpv, 0, 64) : 1.0, pnuc = TP ? __shfl(tpv, 1, 64) : -1.0;
    const bool nuc = TP && pnuc >= 0.0;  // wave-uniform
    const int flags = __shfl(sv, ST_FLAGS, 64), len = __shfl(sv, ST_LEN, 64),
              midx = __shfl(sv, ST_MIDX, 64), nmask = __shfl(sv, ST_NMASK, 64),
              nowhole = __shfl(sv, ST_NOWHOLE, 64), cnt = __shfl(sv, ST_COUNT, 64),
              pos_t = __shfl(sv, ST_POS, 64);
    const int tgt = midx < 64 ? __shfl(tgv, midx, 64) : (int)targets[(long)r * max_masks + midx];
    const int code = grammar_state(flags, len, tgt, nowhole);
    const uint8_t* kp = tk + code * V;
    const uint8_t* rj = tr + code * V;
    // e = exp(where(keep, float64(logit), -100.0) / t); sort keys: the masked
    // float32 logit's order image (the probabilities' order: t > 0, and the
    // division, exp and the two normalisations are monotone and keep distinct
    // float32 inputs distinct) above the index (ties: larger index first)
    uint64_t kv[8];
    if constexpr (!TP) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int i = lane * 8 + j;
        const float x = (i < V && kp[i]) ? lg8[j] : -100.f;
        kv[j] = i < V ? ((uint64_t)f32_ord(x) << 32) | (uint32_t)i : 0ull;
        pe[i] = i < V ? exp((double)x) : 0.;
      }
    } else {
      double xs[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int i = lane * 8 + j;
        const float x = (i < V && kp[i]) ? lg8[j] : -100.f;
        kv[j] = i < V ? ((uint64_t)f32_ord(x) << 32) | (uint32_t)i : 0ull;
        xs[j] = (double)x;
      }
      if (temp != 1.0) {  // wave-uniform; x / 1.0 = x, so t = 1 skips the divisions
#pragma unroll
        for (int j = 0; j < 8; ++j) xs[j] = xs[j] / temp;
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int i = lane * 8 + j;
        pe[i] = i < V ? exp(xs[j]) : 0.;
      }
    }
    __syncthreads();
    SSTAMP(2);
    {
      const double t = np_pairwise_par(pe, V, sp, pwl, lane);
      if (lane == 0) bc[0] = t;
    }
    __syncthreads();
    const double S = bc[0];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int i = lane * 8 + j;
      if (i < V) pe[i] = pe[i] / S;
    }
    __syncthreads();
    SSTAMP(3);
    if (lane == 0) bc[1] = seq_sum(pe, V);
    __syncthreads();
    SSTAMP(4);
    const double T = nuc ? bc[1] + 1e-5 : bc[1];  // nucleus: probs /= (sum(probs) + 1e-5)
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int i = lane * 8 + j;
      if (i < V) pe[i] = pe[i] / T;
    }
    // The sort order, the sorted p and the cdf.  Fast path: the elements
    // with x > -100 (set A: kept logits) sorted alone on a 64 / 128 / 256-key
    // network; the rest all equal -100 (masked, or kept at exactly -100: set
    // B, one shared p) and follow in descending index order, and when some
    // kept logit is >= -60 their p is below 2^-54 of A's sum, so adding them
    // leaves every cdf value past A at t_A: the cdf of A ends at t_A / t_A =
    // 1.0 exactly, every draw u < 1 lands in A, and B is never needed.  Any
    // kept logit below -100, none >= -60, no A, or a pB check that fails
    // takes the full 512-key path (numpy's arithmetic either way).
    // With a temperature the masked elements sit at -100 / t: "some kept
    // logit >= -60" becomes (x + 100) / t >= 40, i.e. x >= -100 + 40 t (pB <=
    // e^-40 of the largest p, below 2^-54; only a filter for rows whose pB
    // check would fail: that check runs on the scaled p themselves).
    // Nucleus: the candidates are a prefix of the sort order and c a
    // sequential sum from its start, so when c at A's last position exceeds
    // p the threshold crossing lies inside A, neither B nor the pB check
    // matters, and A's sort serves; otherwise the full path.
    double cd[8];
    int sidx[8];
    double total;
    bool fast;
    // nucleus, from q in sort order (sp) and c (cq), sort position s = lane *
    // El + e over N positions: the candidates' cdf into cd (-1 past them)
    auto nucleus_cdf = [&](int El, int N) {
      int first = N;
#pragma unroll
      for (int e = 7; e >= 0; --e) {
        const int s = lane * El + e;
        if (e < El && s < N && cq[TP ? s : 0] > pnuc) first = s;
      }
      const uint64_t m = __ballot(first < N);  // s grows with the lane: the lowest lane's is the first
      const int K = m ? __shfl(first, __builtin_ctzll(m), 64) + 1 : N;
      const double den = cq[TP ? K - 1 : 0];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int s = lane * El + e;
        if (e < El && s < K) sp[s] = sp[s] / den;
      }
      __syncthreads();
      if (lane == 0) bc[0] = seq_cumsum(sp, sp, K);
      __syncthreads();
      total = bc[0];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int s = lane * El + e;
        cd[e] = (e < El && s < K) ? sp[s] / total : -1.0;
      }
    };
    {
      uint32_t am = 0u;
      bool c_any = false, hi = false;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int i = lane * 8 + j;
        const float x = (i < V && kp[i]) ? lg8[j] : -100.f;
        if (i < V && x > -100.f) am |= 1u << j;
        if (i < V && x < -100.f) c_any = true;
        if (i < V && (TP ? (double)x >= -100.0 + 40.0 * temp : x >= -60.f)) hi = true;
      }
      fast = !__any(c_any) && (nuc || __any(hi)) && __any(am != 0u);
      if (fast) {
        // compact A's keys into LDS (prefix over lanes), pad to the network size
        int incl = __popc(am);
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
          const int t = __shfl_up(incl, d, 64);
          if (lane >= d) incl += t;
        }
        const int NA = __shfl(incl, 63, 64);
        int pos = incl - __popc(am);
#pragma unroll
        for (int j = 0; j < 8; ++j)
          if (am & (1u << j)) kA[pos++] = kv[j];
        const int E = NA <= 64 ? 1 : NA <= 128 ? 2 : NA <= 256 ? 4 : 8;
        for (int q = NA + lane; q < 64 * E; q += 64) kA[q] = 0ull;  // below every key
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 8; ++j) { cd[j] = -1.0; sidx[j] = 0; }
        if (E == 1) fast_sort_gather<1>(kA, lane, NA, sidx, sp, pe);
        else if (E == 2) fast_sort_gather<2>(kA, lane, NA, sidx, sp, pe);
        else if (E == 4) fast_sort_gather<4>(kA, lane, NA, sidx, sp, pe);
        else fast_sort_gather<8>(kA, lane, NA, sidx, sp, pe);
        // p of a B element (all equal), if any: the first one
        uint32_t bmask = 0u;
#pragma unroll
        for (int j = 0; j < 8; ++j)
          if (lane * 8 + j < V && !(am & (1u << j))) bmask |= 1u << j;
        const uint64_t bm = __ballot(bmask != 0u);
        double pB = 0.;
        if (bm) {
          const int bl = __builtin_ctzll(bm);
          const int bj = __builtin_ctz((uint32_t)__shfl((int)bmask, bl, 64));
          pB = pe[bl * 8 + bj];
        }
        __syncthreads();
        if (lane == 0) bc[0] = seq_cumsum(sp, nuc ? cq : sp, NA);
        __syncthreads();
        SSTAMP(7);
        total = bc[0];
        if (nuc) {
          if (total > pnuc) nucleus_cdf(E, NA);
          else fast = false;  // the crossing is not inside A (or c is NaN)
        } else if (pB * 18014398509481984.0 > total) {  // 2^54: the B terms would not vanish
          fast = false;
        } else {
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const int s = lane * E + e;
            if (e < E && s < NA) cd[e] = sp[s] / total;
          }
        }
      }
    }
    if (!fast) {
      // the full path: bitonic sort of all 512 keys in registers
      sort_desc<8>(kv, lane);
      __syncthreads();
      SSTAMP(5);
      // p in sort order (slot s = lane * 8 + j holds sort position s)
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int s = lane * 8 + j;
        sidx[j] = (int)(uint32_t)kv[j];
        sp[s] = s < V ? pe[sidx[j]] : 0.;
      }
      __syncthreads();
      SSTAMP(6);
      if (lane == 0) bc[0] = seq_cumsum(sp, nuc ? cq : sp, V);
      __syncthreads();
      SSTAMP(7);
      total = bc[0];
      if (nuc) {
        nucleus_cdf(8, V);
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int s = lane * 8 + j;
          cd[j] = s < V ? sp[s] / total : 2.0;
        }
      }
    }
    const bool bad = !(fabs(total - 1.0) <= 1e-9);  // the host path hands such rows to np.random.choice
    // draws (the reference's redraw loop: up to 11 redraws, the last kept):
    // the first sort position whose cdf exceeds u
    auto draw = [&]() -> int {
      const double u = mt_uniform(key, pos, lane);
      int first = 8;
#pragma unroll
      for (int j = 7; j >= 0; --j)
        if (cd[j] > u) first = j;
      const uint64_t m = __ballot(first < 8);
      const int ln = m ? __builtin_ctzll(m) : 63;
      const int fj = __shfl(first, ln, 64);
      int idx = 0;
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (j == (fj < 8 ? fj : 7)) idx = sidx[j];
      return __shfl(idx, ln, 64);
    };
    int idx = draw();
    SSTAMP(8);
    int n = 0;
    bool fail = false;
    while (rj[idx]) {
      idx = draw();
      if (++n > 10) { fail = true; break; }
    }
    if (lane == 0) {
      const bool l = grammar_commit(r, idx, fail, flags, len, midx, nmask, cnt, pos_t, st, tcls, eos, m0,
                                    trash_pos, max_span, src_len, ids, meta, M, out_tok, cap);
      if (bad) st[ST_ERR] |= 2;
      live += l ? 1 : 0;
    }
    __syncthreads();
  }
  SSTAMP(9);
  for (int i = lane; i < 624; i += 64) mt[i] = key[i];
  if (lane == 0) {
    mt[624] = (uint32_t)pos;
    if constexpr (ROWS) {
      if (live) {
        if (RING) __hip_atomic_fetch_add(&alive[0], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        else atomicAdd(alive, 1);  // zeroed by the caller's memset
      }
      if (RING) grammar_ring_ticket(alive, ring, ring_n, R);
    } else if (RING) {
      const int s = alive[2];
      __hip_atomic_store(&ring[s % ring_n], live, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      alive[2] = s + 1;
    } else {
      alive[0] = live;
    }
  }
}

namespace {
int launch_grammar_sample(int R, int V, const float* logits, long ldl, int32_t* state, int nst,
                          const int8_t* targets, int max_masks, const uint8_t* keep, const uint8_t* reject,
                          const uint8_t* cls, int eos, int m0, int trash_pos, int max_span,
                          const int32_t* src_len, int64_t* ids, int32_t* meta, int32_t* out_tok, int cap,
                          uint32_t* mt, long ldmt, bool rows, int32_t* ctl, int32_t* ring, int ring_n,
                          const double* tp, smer_stream_t stream) {
  SMER_REQUIRE(R > 0 && V > 0 && V <= SMX && nst >= 9 && max_masks > 0 && cap > 0,
               "smer_grammar_sample_step[_tp|_rows]: sizes (V <= 512)");
  SMER_REQUIRE(ldl >= V, "smer_grammar_sample_step[_tp|_rows]: logits row stride");
  SMER_REQUIRE(logits && state && targets && keep && reject && cls && src_len && ids && meta && out_tok && mt && ctl,
               "smer_grammar_sample_step[_tp|_rows]: null pointer");
  SMER_REQUIRE(eos >= 0 && eos < V && m0 >= 0 && m0 < V && trash_pos > 0 && max_span > 1,
               "smer_grammar_sample_step[_tp|_rows]: token ids");
  hipStream_t s = (hipStream_t)stream;
  void* dring = nullptr;
  if (ring) {
    if (hipHostGetDevicePointer(&dring, ring, 0) != hipSuccess || dring == nullptr) {
      (void)hipGetLastError();
      dring = ring;
    }
  }
  // rows: one block per request, each on its own stream; without a ring the
  // blocks add themselves to ctl[0], zeroed here (as smer_grammar_greedy_step)
  if (rows && !ring && hipMemsetAsync(ctl, 0, sizeof(int32_t), s) != hipSuccess)
    return smer_set_error(SMER_ERR_HIP, "smer_grammar_sample_step_rows: memset");
  auto go = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, dim3(rows ? R : 1), dim3(64), 0, s, R, V, logits, ldl, state, nst, targets,
                       max_masks, keep, reject, cls, eos, m0, trash_pos, max_span, src_len, ids, meta, 2 * R,
                       out_tok, cap, ctl, (int32_t*)dring, ring ? ring_n : 0, mt, tp, ldmt);
  };
  auto pick = [&](auto rg, auto t) {
    constexpr bool RG = decltype(rg)::value, T = decltype(t)::value;
    if (rows) go(grammar_sample_kernel<RG, T, true>);
    else go(grammar_sample_kernel<RG, T, false>);
  };
  if (ring) {
    if (tp) pick(std::true_type{}, std::true_type{});
    else pick(std::true_type{}, std::false_type{});
  } else {
    if (tp) pick(std::false_type{}, std::true_type{});
    else pick(std::false_type{}, std::false_type{});
  }
  SMER_CHECK_LAUNCH("smer_grammar_sample_step");
  return SMER_OK;
}
}  // namespace

extern "C" int smer_grammar_sample_step(int R, int V, const float* logits, long ldl, int32_t* state,
                                        int nst, const int8_t* targets, int max_masks, const uint8_t* keep,
                                        const uint8_t* reject, const uint8_t* cls, int eos, int m0,
                                        int trash_pos, int max_span, const int32_t* src_len, int64_t* ids,
                                        int32_t* meta, int32_t* out_tok, int cap, uint32_t* mt,
                                        int32_t* ctl, int32_t* ring, int ring_n, smer_stream_t stream) {
  return launch_grammar_sample(R, V, logits, ldl, state, nst, targets, max_masks, keep,
                               reject, cls, eos, m0, trash_pos, max_span, src_len, ids, meta, out_tok, cap, mt,
                               625, false, ctl, ring, ring_n, nullptr, stream);
}

// The same step with a temperature and a nucleus threshold per request: tp
// double [R, 2] on the device (t, p; p < 0 = None), read on every step.
extern "C" int smer_grammar_sample_step_tp(int R, int V, const float* logits, long ldl, int32_t* state,
                                           int nst, const int8_t* targets, int max_masks,
                                           const uint8_t* keep, const uint8_t* reject, const uint8_t* cls,
                                           int eos, int m0, int trash_pos, int max_span,
                                           const int32_t* src_len, int64_t* ids, int32_t* meta,
                                           int32_t* out_tok, int cap, uint32_t* mt, int32_t* ctl,
                                           int32_t* ring, int ring_n, const double* tp,
                                           smer_stream_t stream) {
  SMER_REQUIRE(tp != nullptr, "smer_grammar_sample_step_tp: null tp");
  return launch_grammar_sample(R, V, logits, ldl, state, nst, targets, max_masks,
                               keep, reject, cls, eos, m0, trash_pos, max_span, src_len, ids, meta, out_tok, cap,
                               mt, 625, false, ctl, ring, ring_n, tp, stream);
}

// The same step on one MT19937 stream per request: mt + r * ldmt holds request
// r's 624 key words and position (ldmt >= 625), and the requests run in
// parallel, one block each.  tp may be null: {1.0, None} for every request.
// A request that is done keeps its stream as it is.  The live count: ctl[0]
// (zeroed on the stream here) without a ring, ring[step % ring_n] with one
// (ctl int32 [3] zeroed once by the caller), as smer_grammar_greedy_step[_ring].
extern "C" int smer_grammar_sample_step_rows(int R, int V, const float* logits, long ldl, int32_t* state,
                                             int nst, const int8_t* targets, int max_masks,
                                             const uint8_t* keep, const uint8_t* reject, const uint8_t* cls,
                                             int eos, int m0, int trash_pos, int max_span,
                                             const int32_t* src_len, int64_t* ids, int32_t* meta,
                                             int32_t* out_tok, int cap, uint32_t* mt, long ldmt,
                                             int32_t* ctl, int32_t* ring, int ring_n, const double* tp,
                                             smer_stream_t stream) {
  SMER_REQUIRE(ldmt >= 625, "smer_grammar_sample_step_rows: mt row stride (ldmt >= 625)");
  SMER_REQUIRE(!ring || ring_n > 0, "smer_grammar_sample_step_rows: ring size");
  return launch_grammar_sample(R, V, logits, ldl, state, nst, targets, max_masks,
                               keep, reject, cls, eos, m0, trash_pos, max_span, src_len, ids, meta, out_tok, cap,
                               mt, ldmt, true, ctl, ring, ring_n, tp, stream);
}

// ---------------------------------------------------------------------------
// Per-request pitch constraints: the logits of the tokens a request bans for
// the mask it is about to draw become -100.f before the grammar kernel reads
// them.  Both grammar kernels form x = keep[i] ? logit[i] : -100.f, so a kept
// logit rewritten to exactly -100.f has the x, the sort key and the exp of a
// masked one: the reference's `keep &= ~ban` in sampling().
//   ban_of_mask int8 [R, max_masks]: the ban row of each mask, -1 for none;
//   ban_bits uint32 [R, K, 16]: bit v of row k set = token v is banned.
// One wave per request, 8 tokens per lane (V <= 512).  Done rows, masks with
// no ban row and mask indices past the table leave the row alone; the lookups
// are clamped, not guarded, and only the stores are predicated.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(64) void logits_ban_kernel(
    int R, int V, float* __restrict__ logits, long ldl, const int32_t* __restrict__ state, int nst,
    int max_masks, const int8_t* __restrict__ ban_of_mask, const uint32_t* __restrict__ ban_bits,
    int K) {
  const int r = blockIdx.x, lane = threadIdx.x;
  const int32_t* st = state + (long)r * nst;
  const int done = st[ST_DONE], midx = st[ST_MIDX];
  const int mc = min(max(midx, 0), max_masks - 1);
  const int k = (int)ban_of_mask[(long)r * max_masks + mc];
  const int kc = min(max(k, 0), K - 1);
  // lane's 8 tokens are byte (lane & 3) of word lane / 4
  const uint32_t w = ban_bits[((long)r * K + kc) * 16 + (lane >> 2)];
  const bool on = !done && midx >= 0 && midx < max_masks && k >= 0 && k < K;
  const uint32_t b = on ? (w >> (8 * (lane & 3))) & 0xffu : 0u;
  float* lr = logits + (long)(2 * r + 1) * ldl;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int i = lane * 8 + j;
    if (((b >> j) & 1u) && i < V) lr[i] = -100.f;
  }
}

// Graph-capturable, no allocation, no synchronisation.  logits: the step's
// fp32 logits, request r's row at (2r+1) * ldl (the grammar entries' rows).
extern "C" int smer_logits_ban(int R, int V, float* logits, long ldl, const int32_t* state, int nst,
                               int max_masks, const int8_t* ban_of_mask, const uint32_t* ban_bits,
                               int K, smer_stream_t stream) {
  SMER_REQUIRE(R > 0 && V > 0 && V <= 512 && nst >= 9 && max_masks > 0 && K > 0 && K <= 127,
               "smer_logits_ban: sizes (V <= 512, K <= 127)");
  SMER_REQUIRE(ldl >= V, "smer_logits_ban: logits row stride");
  SMER_REQUIRE(logits && state && ban_of_mask && ban_bits, "smer_logits_ban: null pointer");
  hipLaunchKernelGGL(logits_ban_kernel, dim3(R), dim3(64), 0, (hipStream_t)stream, R, V, logits, ldl,
                     state, nst, max_masks, ban_of_mask, ban_bits, K);
  SMER_CHECK_LAUNCH("smer_logits_ban");
  return SMER_OK;
}

// ---------------------------------------------------------------------------
// Take scores: the log-probability of every drawn token under the model and
// the grammar mask, at t = 1 over the whole distribution (the log of the
// distribution the reference's sampling() builds from the same row:
// generation.token_logprobs).  The logits row lives for one step only, so two
// small kernels bracket the grammar kernel inside the captured step:
//   stage  (after the ban kernel, before the grammar kernel): from the state
//          the step starts in, x_i = keep[code][i] ? (double)logit_i : -100.0,
//          m = max x, lse = m + log(sum exp(x_i - m)) in float64, x_i - lse for
//          i < V into the request's scratch row, and the request's ST_COUNT
//          into its stage slot (-1: the request is done and its scratch row is
//          left alone).  One wave per request, 8 tokens per lane (V <= 512).
//          It writes neither the logits nor the state.
//   commit (after the grammar kernel): a request whose stage slot c is in
//          [0, cap) and whose ST_COUNT is now c + 1 drew out_tok[r, c] in this
//          step: out_lp[r, c] = scratch[r, out_tok[r, c] & 0xFFFF] (bit 16 is
//          the redraw-failure flag).  Nothing else is written.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(64) void logprob_stage_kernel(
    int R, int V, const float* __restrict__ logits, long ldl, const int32_t* __restrict__ state, int nst,
    const int8_t* __restrict__ targets, int max_masks, const uint8_t* __restrict__ keep,
    double* __restrict__ scratch, long ldp, int32_t* __restrict__ stage) {
  const int r = blockIdx.x, lane = threadIdx.x;
  const int32_t* st = state + (long)r * nst;
  const int sv = lane < nst ? st[lane] : 0;
  if (__shfl(sv, ST_DONE, 64)) {  // wave-uniform
    if (lane == 0) stage[r] = -1;
    return;
  }
  const int flags = __shfl(sv, ST_FLAGS, 64), len = __shfl(sv, ST_LEN, 64),
            midx = __shfl(sv, ST_MIDX, 64), nowhole = __shfl(sv, ST_NOWHOLE, 64),
            cnt = __shfl(sv, ST_COUNT, 64);
  // the lookups are clamped (a live request's mask index and state code are
  // in range; a corrupt state must still read inside the tables)
  const int tgt = (int)targets[(long)r * max_masks + min(max(midx, 0), max_masks - 1)];
  const int code = min(max(grammar_state(flags, len, tgt, nowhole), 0), 12);
  const uint8_t* kp = keep + (long)code * V;
  const float* lr = logits + (long)(2 * r + 1) * ldl;
  double x[8];
  double m = -INFINITY;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int i = lane * 8 + j, ic = min(i, V - 1);
    const float lg = lr[ic];
    x[j] = kp[ic] ? (double)lg : -100.0;
    if (i < V) m = fmax(m, x[j]);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmax(m, __shfl_xor(m, o, 64));
  double s = 0.;
#pragma unroll
  for (int j = 0; j < 8; ++j)
    if (lane * 8 + j < V) s += exp(x[j] - m);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);  // a + b = b + a: every lane ends on the same sum
  const double lse = m + log(s);
  double* pr = scratch + (long)r * ldp;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int i = lane * 8 + j;
    if (i < V) pr[i] = x[j] - lse;
  }
  if (lane == 0) stage[r] = cnt;
}

__global__ __launch_bounds__(64) void logprob_commit_kernel(
    int R, int V, const int32_t* __restrict__ state, int nst, const int32_t* __restrict__ stage,
    const int32_t* __restrict__ out_tok, int cap, const double* __restrict__ scratch, long ldp,
    double* __restrict__ out_lp) {
  const int r = blockIdx.x * 64 + threadIdx.x;
  if (r >= R) return;
  const int c = stage[r];
  if (c < 0 || c >= cap || state[(long)r * nst + ST_COUNT] != c + 1) return;
  const int tok = out_tok[(long)r * cap + c] & 0xFFFF;
  if (tok < V) out_lp[(long)r * cap + c] = scratch[(long)r * ldp + tok];
}

// Graph-capturable, no allocation, no synchronisation.  logits, state,
// targets, max_masks and keep are the grammar entry's own arguments.
extern "C" int smer_logprob_stage(int R, int V, const float* logits, long ldl, const int32_t* state, int nst,
                                  const int8_t* targets, int max_masks, const uint8_t* keep, double* scratch,
                                  long ldp, int32_t* stage, smer_stream_t stream) {
  SMER_REQUIRE(R > 0 && V > 0 && V <= 512 && nst >= 9 && nst <= 64 && max_masks > 0,
               "smer_logprob_stage: sizes (V <= 512, 9 <= nst <= 64)");
  SMER_REQUIRE(ldl >= V, "smer_logprob_stage: logits row stride");
  SMER_REQUIRE(ldp >= V, "smer_logprob_stage: scratch row stride");
  SMER_REQUIRE(logits && state && targets && keep && scratch && stage, "smer_logprob_stage: null pointer");
  hipLaunchKernelGGL(logprob_stage_kernel, dim3(R), dim3(64), 0, (hipStream_t)stream, R, V, logits, ldl,
                     state, nst, targets, max_masks, keep, scratch, ldp, stage);
  SMER_CHECK_LAUNCH("smer_logprob_stage");
  return SMER_OK;
}

extern "C" int smer_logprob_commit(int R, int V, const int32_t* state, int nst, const int32_t* stage,
                                   const int32_t* out_tok, int cap, const double* scratch, long ldp,
                                   double* out_lp, smer_stream_t stream) {
  SMER_REQUIRE(R > 0 && V > 0 && V <= 512 && nst >= 9 && cap > 0, "smer_logprob_commit: sizes (V <= 512)");
  SMER_REQUIRE(ldp >= V, "smer_logprob_commit: scratch row stride");
  SMER_REQUIRE(state && stage && out_tok && scratch && out_lp, "smer_logprob_commit: null pointer");
  hipLaunchKernelGGL(logprob_commit_kernel, dim3((R + 63) / 64), dim3(64), 0, (hipStream_t)stream, R, V,
                     state, nst, stage, out_tok, cap, scratch, ldp, out_lp);
  SMER_CHECK_LAUNCH("smer_logprob_commit");
  return SMER_OK;
}

// ---------------------------------------------------------------------------
// Scores of given content: the log-probability of a known token at many rows
// of ONE full (teacher-forced) forward, each row at its own grammar state --
// the number logprob_stage_kernel forms for one live row per request, without
// a step loop or a state vector: the host plan (generation._forced_plan) names
// every scored entry's logits row, state code, ban row and token.
//   x_i = (keep[code][i] && !banned_i) ? (double)logit_i : -100.0,
//   m = max x, lse = m + log(sum exp(x_i - m)) in float64,
//   out_lp[n] = x[id] - lse, out_arg[n] = the first index of the maximum of x
//   (the greedy kernel's rule on the same masked row).
// One wave per entry, 8 tokens per lane (V <= 512); lane l owns tokens 8l ..
// 8l + 7, which are byte l & 3 of ban word l / 4.  x[id] comes from its
// owning lane by shuffle.  Every lookup is clamped (row, code, ban row,
// token), only the two stores are predicated: an entry whose id is outside
// [0, V) or whose row is outside [0, nrows) writes nothing.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(64) void logprob_rows_kernel(
    int N, int V, int nrows, const float* __restrict__ logits, long ldl, const int32_t* __restrict__ row,
    const uint8_t* __restrict__ code, const uint8_t* __restrict__ keep, const int8_t* __restrict__ ban_idx,
    const uint32_t* __restrict__ ban_bits, int K, const int32_t* __restrict__ id,
    double* __restrict__ out_lp, int32_t* __restrict__ out_arg) {
  const int n = blockIdx.x, lane = threadIdx.x;
  const int rw = row[n], tok = id[n], bk = (int)ban_idx[n];
  const int rc = min(max(rw, 0), nrows - 1);
  const int cc = min((int)code[n], 12);
  uint32_t b = 0u;
  if (K > 0) {  // kernel-uniform: with K = 0 the table may be null
    const uint32_t w = ban_bits[(long)min(max(bk, 0), K - 1) * 16 + (lane >> 2)];
    if (bk >= 0 && bk < K) b = (w >> (8 * (lane & 3))) & 0xffu;
  }
  const uint8_t* kp = keep + (long)cc * V;
  const float* lr = logits + (long)rc * ldl;
  double x[8];
  double m = -INFINITY;
  int bi = 0x7fffffff;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int i = lane * 8 + j, ic = min(i, V - 1);
    const float lg = lr[ic];
    x[j] = (kp[ic] && !((b >> j) & 1u)) ? (double)lg : -100.0;
    if (i < V && (x[j] > m || bi == 0x7fffffff)) { m = x[j]; bi = i; }  // ascending i: first max kept
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double om = __shfl_xor(m, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (om > m || (om == m && oi < bi)) { m = om; bi = oi; }  // both partners keep the same pair
  }
  double s = 0.;
#pragma unroll
  for (int j = 0; j < 8; ++j)
    if (lane * 8 + j < V) s += exp(x[j] - m);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);  // a + b = b + a: every lane ends on the same sum
  const double lse = m + log(s);
  const int tc = min(max(tok, 0), V - 1);
  double xt = x[0];
#pragma unroll
  for (int j = 1; j < 8; ++j) xt = (tc & 7) == j ? x[j] : xt;  // selects, no indexed register array
  xt = __shfl(xt, tc >> 3, 64);
  if (lane == 0 && tok >= 0 && tok < V && rw >= 0 && rw < nrows) {
    out_lp[n] = xt - lse;
    out_arg[n] = bi;
  }
}

// Graph-capturable, no allocation, no synchronisation.  logits float32
// [nrows, ldl]; row / code / ban_idx / id / out_lp / out_arg have N entries;
// keep uint8 [13, V]; ban_bits uint32 [K, 16], null allowed when K = 0.
extern "C" int smer_logprob_rows(int N, int V, int nrows, const float* logits, long ldl, const int32_t* row,
                                 const uint8_t* code, const uint8_t* keep, const int8_t* ban_idx,
                                 const uint32_t* ban_bits, int K, const int32_t* id, double* out_lp,
                                 int32_t* out_arg, smer_stream_t stream) {
  SMER_REQUIRE(N > 0 && V > 0 && V <= 512 && nrows > 0 && K >= 0 && K <= 127,
               "smer_logprob_rows: sizes (1 <= V <= 512, 0 <= K <= 127)");
  SMER_REQUIRE(ldl >= V, "smer_logprob_rows: logits row stride");
  SMER_REQUIRE(logits && row && code && keep && ban_idx && id && out_lp && out_arg && (ban_bits || K == 0),
               "smer_logprob_rows: null pointer");
  hipLaunchKernelGGL(logprob_rows_kernel, dim3(N), dim3(64), 0, (hipStream_t)stream, N, V, nrows, logits,
                     ldl, row, code, keep, ban_idx, ban_bits, K, id, out_lp, out_arg);
  SMER_CHECK_LAUNCH("smer_logprob_rows");
  return SMER_OK;
}

// ---------------------------------------------------------------------------
// Infill templates: for the first positions of a span the token, or only its
// class, is given; the row is rewritten so that the grammar kernel can draw
// nothing else.  Both grammar kernels form x = keep[i] ? logit[i] : -100.f, so
// a kept logit stored as exactly -100.f is a masked one, and the forced
// token's 0.f survives because the host validated that its state keeps it.
//   tape int16 [R, max_masks, L]: the entry that governs the draw made when
//   the span holds i body tokens (ST_LEN == i + 1) is tape[r, midx, i]:
//   -1 free, 0 .. V-1 that token, -2 any pitch token (the C_PITCH bit of cls).
// One wave per request, 8 tokens per lane (V <= 512), logits_ban_kernel's
// layout.  A token entry stores 0.f at the token and -100.f at every other
// i < V; -2 stores -100.f at every i < V that is no pitch.  Done rows, free
// entries, a mask index or a position outside the tape and an entry >= V
// write nothing; the lookups are clamped, not guarded, and only the stores
// are predicated.  The class bytes do not depend on the state, so their loads
// run beside the state -> tape chain.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(64) void logits_template_kernel(
    int R, int V, float* __restrict__ logits, long ldl, const int32_t* __restrict__ state, int nst,
    const uint8_t* __restrict__ cls, const int16_t* __restrict__ tape, int max_masks, int L) {
  const int r = blockIdx.x, lane = threadIdx.x;
  const int32_t* st = state + (long)r * nst;
  const int done = st[ST_DONE], midx = st[ST_MIDX], at = st[ST_LEN] - 1;
  const int mc = min(max(midx, 0), max_masks - 1), ac = min(max(at, 0), L - 1);
  const int e = (int)tape[((long)r * max_masks + mc) * L + ac];
  const bool on = !done && midx >= 0 && midx < max_masks && at >= 0 && at < L;
  const bool tok = on && e >= 0 && e < V, pitch = on && e == -2;
  float* lr = logits + (long)(2 * r + 1) * ldl;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int i = lane * 8 + j;
    const bool is_pitch = cls[min(i, V - 1)] & C_PITCH;
    if (i < V && (tok || (pitch && !is_pitch))) lr[i] = (tok && i == e) ? 0.f : -100.f;
  }
}

// Graph-capturable, no allocation, no synchronisation.  logits, state and cls
// are the grammar entry's own arguments (request r's row at (2r+1) * ldl).
extern "C" int smer_logits_template(int R, int V, float* logits, long ldl, const int32_t* state, int nst,
                                    const uint8_t* cls, const int16_t* tape, int max_masks, int L,
                                    smer_stream_t stream) {
  SMER_REQUIRE(R > 0 && V > 0 && V <= 512 && nst >= 9 && max_masks > 0 && L > 0,
               "smer_logits_template: sizes (V <= 512)");
  SMER_REQUIRE(ldl >= V, "smer_logits_template: logits row stride");
  SMER_REQUIRE(logits && state && cls && tape, "smer_logits_template: null pointer");
  hipLaunchKernelGGL(logits_template_kernel, dim3(R), dim3(64), 0, (hipStream_t)stream, R, V, logits, ldl,
                     state, nst, cls, tape, max_masks, L);
  SMER_CHECK_LAUNCH("smer_logits_template");
  return SMER_OK;
}

// ---------------------------------------------------------------------------
// Bar clock (fill_bar=): a note span never passes the bar line and can end
// only when its bar is exactly full.  The first stateful constraint: the node
// follows the tokens drawn, in integers (sixteenths), by the cursor rule of
// codec._Writer -- consecutive duration tokens sum into one group, any other
// token closes an open group, 'sep' rewinds the next group by the previous
// one (generation._BarClock is the host mirror, word for word).
//   clock int32 [R, 8]: T cursor, P previous group's length, A pending
//   duration sum, flags G | S << 1 (a group is open, a 'sep' is pending), seen
//   (the ST_COUNT the clock has followed); words 5..7 unused;
//   units uint8 [V]: a token's length in sixteenths (0: no duration);
//   bar_len int32 [R]: the bar's length L, 0 = the request has no clock.
// Per step, for a request that is not done, with c = ST_COUNT: at the start of
// a span (ST_LEN == 1) the clock is cleared; else, if c == seen + 1 and 1 <= c
// <= cap, it advances by out_tok[r, c - 1] (the token the grammar kernel
// emitted in the step before; bit 16 is the redraw-failure flag); then seen =
// c, so a second launch in one step changes nothing.  With base = S ? T - P : T
// and end = base + A, an active row (not done, L > 0, a note span's mask, c <=
// cap) stores -100.f over
//   a duration of u units iff end + u > L,
//   a pitch, 'continue' and 'rest' iff end >= L (each needs a sixteenth after it),
//   'sep' iff (G ? base : T - P) >= L (where the group after it would start),
//   <eos> and the control tokens (which end a note span) iff end != L.
// Both grammar kernels form x = keep[i] ? logit[i] : -100.f, so a kept logit
// stored as exactly -100.f is a masked one (logits_ban_kernel's argument).
// One wave per request, 8 tokens per lane (V <= 512), logits_ban_kernel's
// layout.  The lookups are clamped, not guarded, and only the stores are
// predicated; a done row stores nothing at all, and a row whose count has run
// past out_tok (c > cap: its clock missed a token) stores no logit.  The
// candidates' class and unit bytes do not depend on the state, so their loads
// run beside the state -> out_tok -> class / units chain.
// ---------------------------------------------------------------------------
namespace {
constexpr int CK_WORDS = 8;
}  // namespace

__global__ __launch_bounds__(64) void bar_clock_kernel(
    int R, int V, float* __restrict__ logits, long ldl, const int32_t* __restrict__ state, int nst,
    const int8_t* __restrict__ targets, int max_masks, const int32_t* __restrict__ out_tok, int cap,
    const uint8_t* __restrict__ cls, const uint8_t* __restrict__ units, int eos,
    const int32_t* __restrict__ bar_len, int32_t* __restrict__ clock) {
  const int r = blockIdx.x, lane = threadIdx.x;
  const int32_t* st = state + (long)r * nst;
  const int done = st[ST_DONE], midx = st[ST_MIDX], len = st[ST_LEN], c = st[ST_COUNT];
  int32_t* ck = clock + (long)r * CK_WORDS;
  const int cv = ck[lane & (CK_WORDS - 1)];  // lane k <- word k, then broadcast
  int T = __shfl(cv, 0, 64), P = __shfl(cv, 1, 64), A = __shfl(cv, 2, 64);
  const int fl = __shfl(cv, 3, 64), seen = __shfl(cv, 4, 64);
  int G = fl & 1, S = (fl >> 1) & 1;
  const int L = bar_len[r];
  const int tgt = (int)targets[(long)r * max_masks + min(max(midx, 0), max_masks - 1)];
  const int tok = out_tok[(long)r * cap + min(max(c - 1, 0), cap - 1)] & 0xFFFF;
  const int tcls = cls[min(tok, V - 1)], tun = units[min(tok, V - 1)];
  if (len == 1) {
    T = P = A = G = S = 0;
  } else if (c == seen + 1 && c >= 1 && c <= cap && tok < V) {
    if (tcls & C_DUR) {
      A += tun;
      G = 1;
    } else {
      if (G) {  // _Writer.flush
        T = (S ? T - P : T) + A;
        P = A;
        A = S = G = 0;
      }
      if (tcls & C_SEPSTR) S = 1;
    }
  }
  if (!done && lane < 5)
    ck[lane] = lane == 0 ? T : lane == 1 ? P : lane == 2 ? A : lane == 3 ? (G | (S << 1)) : c;
  const int base = S ? T - P : T, end = base + A, sep_base = G ? base : T - P;
  const bool on = !done && L > 0 && midx >= 0 && midx < max_masks && tgt == 0 && c <= cap;
  float* lr = logits + (long)(2 * r + 1) * ldl;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int i = lane * 8 + j, ic = min(i, V - 1);
    const int cb = cls[ic], u = units[ic];
    const bool ban = ((cb & C_DUR) && end + u > L) ||
                     ((cb & (C_PITCH | C_CONT | C_RESTSTR)) && end >= L) ||
                     ((cb & C_SEPSTR) && sep_base >= L) ||
                     (((cb & C_CTRL) || i == eos) && end != L);
    if (on && ban && i < V) lr[i] = -100.f;
  }
}

// Graph-capturable, no allocation, no synchronisation.  logits, state,
// targets, out_tok and cls are the grammar entry's own arguments (request r's
// row at (2r+1) * ldl); the caller zeroes `clock` once per decode.
extern "C" int smer_bar_clock(int R, int V, float* logits, long ldl, const int32_t* state, int nst,
                              const int8_t* targets, int max_masks, const int32_t* out_tok, int cap,
                              const uint8_t* cls, const uint8_t* units, int eos, const int32_t* bar_len,
                              int32_t* clock, smer_stream_t stream) {
  SMER_REQUIRE(R > 0 && V > 0 && V <= 512 && nst >= 9 && max_masks > 0 && cap > 0,
               "smer_bar_clock: sizes (V <= 512)");
  SMER_REQUIRE(ldl >= V, "smer_bar_clock: logits row stride");
  SMER_REQUIRE(eos >= 0 && eos < V, "smer_bar_clock: token ids");
  SMER_REQUIRE(logits && state && targets && out_tok && cls && units && bar_len && clock,
               "smer_bar_clock: null pointer");
  hipLaunchKernelGGL(bar_clock_kernel, dim3(R), dim3(64), 0, (hipStream_t)stream, R, V, logits, ldl, state,
                     nst, targets, max_masks, out_tok, cap, cls, units, eos, bar_len, clock);
  SMER_CHECK_LAUNCH("smer_bar_clock");
  return SMER_OK;
}

// ---------------------------------------------------------------------------
// Chord-following infill (chords=): the pitch set a note may use depends on
// where in its bar the note starts.  The bar clock's end = base + A (base = S ?
// T - P : T) is exactly the onset of a pitch drawn next: a pitch is no duration
// token, so it first closes an open group (T' = base + A) and sounds at the new
// group's base, which is T'; with no group open A is 0 and the onset is base.
// So a pitch after 'sep' reads the rewound position, and the second pitch of a
// chord the first one's.  The node only reads the clock words smer_bar_clock
// left in this same step (T, P, A, G | S << 1); it never writes them.
//   chord_len int32 [R]: the bar's length L_r in sixteenths, 0 = no chords;
//   chord_at int8 [R, max_masks, 64]: the bit row that governs each position
//   of each mask's bar, -1 for none;
//   chord_bits uint32 [R, 16, 16]: bit v of row k set = token v is banned
//   (ban_bits' layout).
// pos = min(max(end, 0), min(L_r, 64) - 1); k = chord_at[r, midx, pos].  A row
// is active iff it is not done, L_r > 0, 0 <= midx < max_masks, its target is 0
// (a note span), c = ST_COUNT <= cap and 0 <= k < 16; it stores -100.f over the
// set bits of row k at i < V in logits row 2r + 1.  Everything else writes
// nothing.  One wave per request, 8 tokens per lane (V <= 512),
// logits_ban_kernel's layout; the lookups are clamped, not guarded, and only
// the stores are predicated.
// ---------------------------------------------------------------------------
namespace {
constexpr int CHORD_POS = 64, CHORD_ROWS = 16;
}  // namespace

__global__ __launch_bounds__(64) void chord_ban_kernel(
    int R, int V, float* __restrict__ logits, long ldl, const int32_t* __restrict__ state, int nst,
    const int8_t* __restrict__ targets, int max_masks, int cap, const int32_t* __restrict__ clock,
    const int32_t* __restrict__ chord_len, const int8_t* __restrict__ chord_at,
    const uint32_t* __restrict__ chord_bits) {
  const int r = blockIdx.x, lane = threadIdx.x;
  const int32_t* st = state + (long)r * nst;
  const int done = st[ST_DONE], midx = st[ST_MIDX], c = st[ST_COUNT];
  const int cv = clock[(long)r * CK_WORDS + (lane & (CK_WORDS - 1))];  // lane k <- word k, then broadcast
  const int T = __shfl(cv, 0, 64), P = __shfl(cv, 1, 64), A = __shfl(cv, 2, 64);
  const int S = (__shfl(cv, 3, 64) >> 1) & 1;
  const int end = (S ? T - P : T) + A;
  const int L = chord_len[r];
  const int pos = max(min(max(end, 0), min(L, CHORD_POS) - 1), 0);
  const long m = (long)r * max_masks + min(max(midx, 0), max_masks - 1);
  const int tgt = (int)targets[m];
  const int k = (int)chord_at[m * CHORD_POS + pos];
  const int kc = min(max(k, 0), CHORD_ROWS - 1);
  // lane's 8 tokens are byte (lane & 3) of word lane / 4
  const uint32_t w = chord_bits[((long)r * CHORD_ROWS + kc) * 16 + (lane >> 2)];
  const bool on = !done && L > 0 && midx >= 0 && midx < max_masks && tgt == 0 && c <= cap && k >= 0 &&
                  k < CHORD_ROWS;
  const uint32_t b = on ? (w >> (8 * (lane & 3))) & 0xffu : 0u;
  float* lr = logits + (long)(2 * r + 1) * ldl;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int i = lane * 8 + j;
    if (((b >> j) & 1u) && i < V) lr[i] = -100.f;
  }
}

// Graph-capturable, no allocation, no synchronisation.  logits, state, targets
// and cap are the grammar entry's own arguments (request r's row at (2r+1) *
// ldl); clock is smer_bar_clock's, which runs ahead of this entry in the step.
extern "C" int smer_chord_ban(int R, int V, float* logits, long ldl, const int32_t* state, int nst,
                              const int8_t* targets, int max_masks, int cap, const int32_t* clock,
                              const int32_t* chord_len, const int8_t* chord_at, const uint32_t* chord_bits,
                              smer_stream_t stream) {
  SMER_REQUIRE(R > 0 && V > 0 && V <= 512 && nst >= 9 && max_masks > 0 && cap > 0,
               "smer_chord_ban: sizes (V <= 512)");
  SMER_REQUIRE(ldl >= V, "smer_chord_ban: logits row stride");
  SMER_REQUIRE(logits && state && targets && clock && chord_len && chord_at && chord_bits,
               "smer_chord_ban: null pointer");
  hipLaunchKernelGGL(chord_ban_kernel, dim3(R), dim3(64), 0, (hipStream_t)stream, R, V, logits, ldl, state,
                     nst, targets, max_masks, cap, clock, chord_len, chord_at, chord_bits);
  SMER_CHECK_LAUNCH("smer_chord_ban");
  return SMER_OK;
}
