// The GEMM dispatch of gemm.hip as a pure function: which kernel a smer_gemm /
// smer_gemm_wgrad_bias_ex / smer_gemm_fp8* / smer_gemm_wgrad_fp8 call runs on,
// with which grid, LDS size and split-K slices.  Plain C++17, no HIP and no environment: the launchers fill a
// GemmQuery, read the switches once per call (gemm_switches, gemm.hip) and
// launch what gemm_plan returns; smer_gemm_plan answers the same question
// without launching (tests/gemmref.py's mirror is held against it).
#ifndef SMER_GEMM_PLAN_H
#define SMER_GEMM_PLAN_H

#include <algorithm>
#include <cstddef>

// tile geometry the plan shares with the kernels (gemm.hip static_asserts
// its own constants against these)
namespace gp {
constexpr int BM = 128, BN = 128, BK = 64;        // 128x128 kernel
constexpr int TILE_BYTES = BM * BK * 2;
constexpr int G64_STAGE = 64 * BK * 2 + TILE_BYTES;
constexpr int G2 = 256, G2K = 64;                 // 256x256 kernels
constexpr int G2_STAGE = 2 * G2 * G2K * 2;
constexpr int G2_LDS = 2 * G2_STAGE + 64 * G2 * 2;
constexpr int GS_KS = 32;                         // staggered 256x256 kernels
constexpr int GS_SLOT = 2 * G2 * GS_KS * 2;
constexpr int SK_BM = 64, SK_BN = 16;             // skinny bf16
constexpr int SKF_BN = 4, SKF_BM = 16, SKF_NW = 4, SKF_UNR = 8;  // skinny fp32
constexpr size_t TICKET_BYTES = 64 * 1024;        // split-K tickets at the end of a workspace
constexpr int LNR_MAXC = 4;                       // LayerNorm-prologue Linear: 16-B row chunks per lane
}  // namespace gp

// Every value the dispatch takes from the environment, at its default.
// "per call" switches are re-read on every call (tests and A/B tools flip
// them in-process); the others are read once per process.
struct GemmSwitches {
  // per call
  bool gemm256 = true;       // SMER_GEMM256=0: no 256x256 forward / dgrad
  int gemm256s = -1;         // SMER_GEMM256S=1 / 0: staggered kernel on / off; -1: K >= 1024 or NN with N >= 1024
  // SMER_G256_NONPERSIST: 1 = the NN dgrad shapes of the 256x256 kernels run
  // one workgroup per tile (grid = tiles) instead of a persistent grid of one
  // per CU, so the hardware dispatcher balances tiles onto the CUs the
  // side-stream weight gradients leave free; 2 = every 256x256 forward /
  // dgrad; 0 = persistent everywhere
  int g256_nonpersist = 0;
  int g256_skew = 0;         // SMER_G256_SKEW, 0..64 (GemmEpi.skew)
  bool gemm64 = true;        // SMER_GEMM64=0: mid-size shapes stay on the 128x128 kernel
  bool wgrad256s = true;     // SMER_WGRAD256S=0: the two-stage 256x256 weight gradient
  bool splitk_fused = false; // SMER_SPLITK_FUSED=1: last-arriver reduction
  bool f32_mfma = true;      // SMER_GEMM_F32_MFMA=0: fp32 NT shapes on the VALU tile kernel
  bool fp8_q8_fast = true;   // SMER_FP8_Q8_FAST=0: e4m3-copy fp8 products on the generic epilogue
  bool gemm256s_fp8 = false; // SMER_GEMM256S_FP8=1: the staggered fp8 kernel
  // once per process
  bool gemm_glds = true;     // SMER_GEMM_GLDS=0: register staging everywhere
  // SMER_WGRAD_GLDS=0: register staging for the 128x128 weight gradients
  // (round 5's workaround; A/B runs).  LDS-DMA since round 6: the
  // non-repeatable overlapped step was the packed-FP32 fault (DESIGN.md
  // section 8), not this kernel, and the library no longer contains
  // packed-FP32 instructions
  bool wgrad_glds = true;
  int splitk_depth = 1024;   // SMER_SPLITK_DEPTH (>= 64): minimum K depth of a 128x128 split-K slice
  int wgrad256 = 2;          // SMER_WGRAD256: 2 = outputs >= 1536 x 768 or both sides >= 768, 1 = every shape, 0 = never
  long wgrad256_slots = 0;   // SMER_WGRAD256_SLOTS (>= 8): work items of the 256x256 weight gradient; 0 = one per CU
  int wgrad256_depth = 512;  // SMER_WGRAD256_DEPTH (>= 64): minimum K depth of its slices
  bool skinny16 = true;      // SMER_SKINNY16=0: 64-row strips only
  int skinny16_cap = 2;      // SMER_SKINNY16_CAP (>= 1): 16-row workgroups per CU
  // SMER_WGRAD_WGP2 (1..4): resident 128x128 split-K workgroups per 2 CUs.
  // 4 = two per CU, the default since round 6 (with the LDS-DMA weight
  // gradient back the overlapped C2 step is the same, 13.09-13.13 vs
  // 13.08-13.10 ms, and the serialised weight gradients run faster: GEMM
  // family 0.244 vs 0.226 of peak); 2 = one per CU (round 5: C2 13.49 vs
  // 13.56 ms with register staging); 1 = one per two CUs.  The weight
  // gradients run on a second stream beside the main chain: a smaller
  // persistent grid leaves CUs (and LDS) to the main stream's kernels and
  // cuts the split-K slab bytes in proportion
  int wgrad_wgp2 = 4;
  long g256_min = 0;         // SMER_G256_MIN (>= 1): fewest tiles for the 256x256 forward; 0 = one per CU
  bool skinny_kf = true;     // SMER_SKINNY_KF=0: the skinny kernels' guarded loads at every K
  bool skinny_rows_f32 = true;  // SMER_SKINNY_ROWS_F32=0: fp32 <= 64-row Linears on gemm_skinny_f32_kernel
};

struct GemmQuery {
  bool f32 = false;  // else bf16
  bool f8 = false;   // e4m3 operands (smer_gemm_fp8*, smer_gemm_wgrad_fp8); excludes f32
  bool ak = true, bk = true;
  int M = 0, N = 0, K = 0;
  // what the dispatch reads of the epilogue (GemmEpi)
  bool C = false, Cf = false, bias = false, relu = false, drop = false, residual = false, gate = false;
  bool vec = false, kv = false, q8 = false;
  bool gate8 = false;        // fp8: the gate is an e4m3 copy (smer_gemm_fp8_gate8)
  long ldcf = 0;
  bool cf_aligned16 = false;
  bool rowsum = false;       // the fused bias gradient (smer_gemm_wgrad_bias_ex)
  bool ws = false;           // a workspace is passed
  size_t ws_bytes = 0;
  bool f32_aligned = false;  // fp32: lda, ldb % 4 == 0 and A, B 16-B aligned
  int cus = 256;
  int max_workgroups = 0;    // cap on the persistent weight-gradient grids; 0 = none
};

// names: tests/gemmref.py KERNEL_NAMES, in its order (smer_gemm_kernel_name)
enum GemmKernel {
  GK_SKINNY_M16_KF, GK_SKINNY_M16_GUARD, GK_SKINNY_S64_KF, GK_SKINNY_S64_GUARD, GK_GEMM64,
  GK_G128_GLDS, GK_G128_REG, GK_G256_STREAM, GK_G256_GENERIC, GK_G256S, GK_SPLITK_REDUCE,
  GK_SPLITK_FUSED, GK_WGRAD256, GK_WGRAD256S, GK_F32_ROWS, GK_F32_SKINNY, GK_F32_MFMA, GK_F32_TILE,
  // gemm256_fp8_kernel<STREAM, Q8, GATE8>, gemm256s_fp8_kernel, gemm256s_wgrad_fp8_kernel
  GK_F8_GENERIC, GK_F8_STREAM, GK_F8_Q8_GENERIC, GK_F8_Q8_STREAM, GK_F8_Q8_GATE8, GK_F8_G256S, GK_F8_WGRAD256S,
  GK_COUNT
};
constexpr int GK_NONE = -1;

inline const char* gemm_kernel_name(int k) {
  static const char* const names[GK_COUNT] = {
      "skinny_m16_kf", "skinny_m16_guard", "skinny_s64_kf", "skinny_s64_guard", "gemm64",
      "g128_glds", "g128_reg", "g256_stream", "g256_generic", "g256s", "splitk_reduce",
      "splitk_fused", "wgrad256", "wgrad256s", "f32_rows", "f32_skinny", "f32_mfma", "f32_tile",
      "f8_generic", "f8_stream", "f8_q8_generic", "f8_q8_stream", "f8_q8_gate8", "f8_g256s", "f8_wgrad256s"};
  return k >= 0 && k < GK_COUNT ? names[k] : nullptr;
}

struct GemmPlan {
  int kernel = GK_NONE;
  bool ak = true, bk = true;  // template arguments beside the kernel
  bool unroll4 = false;       // skinny bf16: 4 k-steps per wave in flight (K > 512), else 2
  int grid_x = 1, grid_y = 1, block = 256;
  size_t lds = 0;             // dynamic LDS bytes
  int split = 1, kchunk = 0;  // split-K slices and their K depth (kchunk = K unsplit)
  int reduce = GK_NONE;       // GK_SPLITK_REDUCE (separate kernel), GK_SPLITK_FUSED (tickets) or none
  size_t rs_offset = 0;       // row-sum partials in the workspace, in floats (split > 1 with rowsum; fp8: split > 1)
};

namespace gp {
inline long cdiv(long a, long b) { return (a + b - 1) / b; }

// max_workgroups applied to a persistent weight-gradient grid
inline long cap(int max_workgroups, long v) {
  return max_workgroups > 0 ? std::max(8L, std::min<long>(v, max_workgroups)) : v;
}

// Deterministic split-K of a weight gradient: `slots` work items over
// `tiles` output tiles, slices at least `depth` deep and whole multiples of
// `granule`, slabs of M * N floats plus `rs_rows` x M floats of row-sum
// partials per slice within the workspace (its tickets excluded), at most 64
// slices.
struct SplitK { long slices; int split, kchunk; };
inline SplitK splitk(const GemmQuery& q, long slots, long tiles, int depth, int granule, int rs_rows) {
  const size_t ws_bytes = q.ws ? q.ws_bytes : 0;
  const size_t slab_bytes = ws_bytes > TICKET_BYTES ? ws_bytes - TICKET_BYTES : 0;
  long s = std::min<long>(slots / std::max<long>(1, tiles), q.K / depth);
  s = std::min<long>(s, (long)(slab_bytes / (((size_t)q.M * q.N + (size_t)rs_rows * q.M) * sizeof(float))));
  s = std::max<long>(1, std::min<long>(s, 64));
  SplitK r{s, 1, q.K};
  if (s > 1) {
    r.kchunk = (int)(cdiv(cdiv(q.K, s), granule) * granule);
    r.split = (int)cdiv(q.K, r.kchunk);
  }
  return r;
}

inline void set_split(GemmPlan& p, const GemmQuery& q, const SplitK& sk, int reduce) {
  p.split = sk.split;
  p.kchunk = sk.kchunk;
  if (sk.split > 1) {
    p.reduce = reduce;
    if (q.rowsum) p.rs_offset = (size_t)sk.split * q.M * q.N;
  }
}

inline GemmPlan plan_f32(const GemmQuery& q, const GemmSwitches& sw) {
  GemmPlan p;
  p.ak = q.ak; p.bk = q.bk; p.kchunk = q.K;
  const bool al = q.ak && q.bk && q.K % 4 == 0 && q.f32_aligned;
  if (al && q.M <= 64) {
    p.grid_x = (int)cdiv(q.N, SKF_BN);
    p.grid_y = (int)cdiv(q.M, SKF_BM);
    p.block = 64 * SKF_NW;
    if (q.K <= SKF_NW * SKF_UNR * 64 && sw.skinny_rows_f32) {
      p.kernel = GK_F32_ROWS;
      p.lds = (size_t)std::min(q.M, SKF_BM) * q.K * sizeof(float);
    } else {
      p.kernel = GK_F32_SKINNY;
    }
    return p;
  }
  p.grid_x = (int)cdiv(q.N, 64);
  p.grid_y = (int)cdiv(q.M, 64);
  p.kernel = al && sw.f32_mfma ? GK_F32_MFMA : GK_F32_TILE;
  return p;
}

// e4m3 operands (the launchers refuse anything but M, N % 256 == 0 and
// K % 128 == 0 forward / K % 64 == 0 weight gradient before they ask): whole
// 256x256 tiles, a persistent grid past one tile per CU.
inline GemmPlan plan_f8(const GemmQuery& q, const GemmSwitches& sw) {
  GemmPlan p;
  p.ak = q.ak; p.bk = q.bk; p.kchunk = q.K;
  p.block = 512;
  const long cus = q.cus, tiles = (long)(q.M / G2) * (q.N / G2);
  if (!q.ak && !q.bk) {
    // weight gradient: the split-K of the bf16 GK_WGRAD256S branch, a slice
    // carrying N / 256 x M bias partials (one row per column tile) whether
    // or not the bias gradient is asked for
    const long slots = cap(q.max_workgroups, sw.wgrad256_slots ? sw.wgrad256_slots : cus);
    const SplitK sk = splitk(q, slots, tiles, sw.wgrad256_depth, G2K, q.N / G2);
    p.kernel = GK_F8_WGRAD256S;
    p.lds = 4 * GS_SLOT;
    p.split = sk.split;
    p.kchunk = sk.kchunk;
    if (sk.split > 1) {
      p.reduce = GK_SPLITK_REDUCE;
      p.rs_offset = (size_t)sk.split * q.M * q.N;
    }
    const long nwg = tiles * sk.split, gcap = cap(q.max_workgroups, cus);
    p.grid_x = nwg > gcap ? (int)(gcap & ~7L) : (int)nwg;
    return p;
  }
  p.grid_x = tiles > cus ? (int)(cus & ~7L) : (int)tiles;
  // The staggered fp8 kernel for whole-tile bf16-output products: opt-in
  // (SMER_GEMM256S_FP8=1 / 0 forces it on / off, read per call).  Isolated
  // and warm (tools/gemm256s_fp8_ab.py, C4 rows 65536, operands re-used across
  // iterations) it wins at K >= 1024 (FFN2 forward 122.3 vs 133.1 us, FFN1 /
  // QKV dgrads 113.8 / 125.1 vs 123.0 / 131.7) and loses at K = 768 (QKV
  // forward 160.7 vs 151.7); inside the C4 fp8 train step, whose operands
  // arrive cold from HBM, the same K >= 1024 calls ran slower (paired
  // kernel trace: 133.5 vs 129.3 us at the 130-us shapes, 794 vs 698 at the
  // vocabulary-long K) and the step did not move (86.3 vs 85.9 ms), so the
  // two-stage kernel stays the default.
  // The e4m3-copy products (the gated FFN2 dgrad, FFN1 with SMER_FP8_FFN2)
  // on the streamed epilogue, whose residual / gate rows arrive by LDS-DMA a
  // pass ahead, one item at a time (round 6: C4 gated dgrad 65536 x 2048 x
  // 768 301 -> 245 us, step 78.96-78.99 -> 78.48-78.57 ms); SMER_FP8_Q8_FAST=0
  // (read per call) keeps the generic epilogue, whose gate loads are a
  // dependent HBM round trip per pass
  if (q.vec && !q.q8 && q.K % G2K == 0 && q.K / G2K >= 4 && sw.gemm256s_fp8) p.kernel = GK_F8_G256S;
  else if (!q.vec) p.kernel = GK_F8_GENERIC;  // (q8 and gate8 require vec)
  else if (q.gate8) p.kernel = GK_F8_Q8_GATE8;
  else if (q.q8) p.kernel = sw.fp8_q8_fast ? GK_F8_Q8_STREAM : GK_F8_Q8_GENERIC;
  else p.kernel = GK_F8_STREAM;
  // the generic epilogues need no epilogue rows in LDS
  p.lds = p.kernel == GK_F8_GENERIC || p.kernel == GK_F8_Q8_GENERIC ? 2 * G2_STAGE : G2_LDS;
  return p;
}
}  // namespace gp

inline GemmPlan gemm_plan(const GemmQuery& q, const GemmSwitches& sw) {
  using namespace gp;
  if (q.f32) return plan_f32(q, sw);
  if (q.f8) return plan_f8(q, sw);
  const int M = q.M, N = q.N, K = q.K;
  const long cus = q.cus;
  GemmPlan p;
  p.ak = q.ak; p.bk = q.bk; p.kchunk = K;
  // decode / small-batch Linears: the skinny kernel
  if (q.ak && q.bk && M <= 4 * SK_BM && !q.rowsum) {
    const long ntn = cdiv(N, SK_BN);
    // 16-row workgroups while that keeps the grid within two per CU
    // (per-workgroup load time, not the grid, bounds a decode Linear)
    const bool m16 = sw.skinny16 && ntn * cdiv(M, 16) <= (long)sw.skinny16_cap * cus;
    const bool kf = K % 32 == 0 && sw.skinny_kf;
    p.kernel = m16 ? (kf ? GK_SKINNY_M16_KF : GK_SKINNY_M16_GUARD) : (kf ? GK_SKINNY_S64_KF : GK_SKINNY_S64_GUARD);
    p.unroll4 = cdiv(K, 32) > 16;  // 8 waves x 4 steps (16 waves would spill at 128 VGPRs)
    p.grid_x = (int)ntn;
    p.grid_y = (int)cdiv(M, m16 ? 16 : SK_BM);
    p.block = 512;
    return p;
  }
  const long t2 = cdiv(M, G2) * cdiv(N, G2);
  const bool whole2 = M % G2 == 0 && N % G2 == 0;
  // large-M forward / dgrad: 256x256 tiles when they fill the chip
  if (q.ak && !q.rowsum && K % G2K == 0 && sw.gemm256 && t2 >= (sw.g256_min ? sw.g256_min : cus)) {
    // whole tiles, bf16 C only, at most one of residual / gate: the streamed
    // epilogue; of those, the staggered kernel where it measured faster
    // (tools/gemm256s_ab.py, round 4): K >= 1024 (C2 FFN2 forward 69.7 vs
    // 73.3 us, FFN1 / QKV dgrads 66.0 / 52.6 vs 71.1 / 56.6) and the NN
    // dgrads with N >= 1024 (gated FFN2 dgrad 104.8 vs 116.9); the K = 512
    // forwards keep the two-stage kernel (their epilogue sets the time)
    const bool stream = q.vec && q.C && !q.Cf && !q.kv && whole2 && !(q.residual && q.gate);
    const bool stag = sw.gemm256s == 1 || (sw.gemm256s != 0 && (K >= 1024 || (!q.bk && N >= 1024)));
    if (stag && stream && !q.q8 && K % GS_KS == 0 && K / GS_KS >= 4) p.kernel = GK_G256S;
    else p.kernel = stream ? GK_G256_STREAM : GK_G256_GENERIC;
    // persistent (one workgroup per CU) unless SMER_G256_NONPERSIST
    const bool per_tile = sw.g256_nonpersist == 2 || (sw.g256_nonpersist == 1 && !q.bk);
    p.grid_x = (t2 > cus && !per_tile) ? (int)(cus & ~7L) : (int)t2;
    p.block = 512;
    p.lds = G2_LDS;
    return p;
  }
  const bool cf_only = q.Cf && !q.C && !q.bias && !q.residual && !q.gate && !q.relu && !q.drop &&
                       ((long)M * N) % 4 == 0;
  // weight gradients (both operands column images, pure fp32 output): the
  // 256x256 tile when its split-K fills the chip with >= 512-deep slices.
  // Outputs with both sides >= 768 (or >= 1536 x 768) take it: every C4
  // weight gradient (tools/bench_wgrad.py c4: 3072x768x65536 350 vs 426 us;
  // C4 fp8 step 84.5-85.0 vs 85.6-86.3 ms), no C2 one (at 512-wide outputs
  // the 128x128 kernel with its smaller slabs is as fast or faster: C2
  // 13.08-13.16 vs 13.19-13.22 ms).  The staggered schedule is the faster of
  // its two kernels (2304x768x65536 249 vs 284 us)
  const bool big = sw.wgrad256 == 1 ||
                   (sw.wgrad256 == 2 && ((long)M * N >= 1536L * 768 || (M >= 768 && N >= 768)));
  if (!q.ak && !q.bk && K % G2K == 0 && q.ws && big) {
    const long slots = cap(q.max_workgroups, sw.wgrad256_slots ? sw.wgrad256_slots : cus);
    const SplitK sk = splitk(q, slots, t2, sw.wgrad256_depth, G2K, 1);
    if (cf_only && t2 * sk.slices * 4 >= 3 * cus) {
      const bool stag = sw.wgrad256s && whole2 && q.vec;
      p.kernel = stag ? GK_WGRAD256S : GK_WGRAD256;
      p.lds = stag ? 4 * GS_SLOT : 2 * G2_STAGE;
      set_split(p, q, sk, GK_SPLITK_REDUCE);
      const long nwg = t2 * sk.split, gcap = cap(q.max_workgroups, cus);
      p.grid_x = nwg > gcap ? (int)(gcap & ~7L) : (int)nwg;
      p.block = 512;
      return p;
    }
  }
  // the 128x128 kernel; a pure Cf (+)= A.B^T epilogue with few output tiles
  // and a long K splits K over ~2 resident workgroups per CU (more slices
  // only add slab traffic; floor: a partial second wave of workgroups costs
  // a whole slice time)
  const int tiles = (int)(cdiv(M, BM) * cdiv(N, BN));
  const long resident = cap(q.max_workgroups, std::max(8L, sw.wgrad_wgp2 * cus / 2));
  SplitK sk{1, 1, K};
  if (cf_only && tiles < 512 && K >= 1024) sk = splitk(q, resident, tiles, sw.splitk_depth, BK, 1);
  // mid-size forward / dgrad: fewer 128x128 tiles than two per CU -> 64x128
  if (q.ak && !q.rowsum && sk.split == 1 && K % BK == 0 && tiles <= 4 * cus && M > 4 * SK_BM &&
      sw.gemm_glds && sw.gemm64) {
    const long t64 = cdiv(M, 64) * cdiv(N, BN), res = 3 * cus;
    p.kernel = GK_GEMM64;
    p.grid_x = t64 > res ? (int)(res & ~7L) : (int)t64;
    p.lds = 2 * G64_STAGE;
    return p;
  }
  // fused split-K reduction by the tile's last-arriving slice (no separate
  // reduce launch): whole float4 rows of dW.  Off by default: C2 step
  // 13.64-16.62 ms fused vs 13.04-13.09 separate (every slice waits for its
  // write-through slab stores before taking the ticket, and the last
  // arriver sums the tile alone); bit-identical either way
  const bool fused = sw.splitk_fused && (N & 3) == 0 && (q.ldcf & 3) == 0 && q.cf_aligned16 &&
                     (size_t)tiles * 4 <= TICKET_BYTES && q.ws_bytes >= TICKET_BYTES;
  set_split(p, q, sk, fused ? GK_SPLITK_FUSED : GK_SPLITK_REDUCE);
  // persistent grid: two resident workgroups per CU (LDS 64 KiB, <= 256
  // VGPRs), the split-K weight gradients SMER_WGRAD_WGP2 per two
  const long nwg = (long)tiles * sk.split, fit = sk.split > 1 ? resident : 2 * cus;
  p.grid_x = nwg > fit ? (int)(fit & ~7L) : (int)nwg;
  // LDS-DMA staging needs whole 64-deep K steps in every slice
  const bool gl = K % BK == 0 && sk.kchunk % BK == 0 && sw.gemm_glds && (q.ak || q.bk || sw.wgrad_glds);
  p.kernel = gl ? GK_G128_GLDS : GK_G128_REG;
  p.lds = 4 * TILE_BYTES;
  return p;
}

// smer_linear_decode_ln's gemm_skinny_ln_kernel<8, UNR, NC, KF>: the K-full
// forms by row length, else the guarded loads with 4 k-steps in flight past
// 16 steps (smer_linear_decode_ln_plan)
struct SklnPlan { int UNR, NC; bool KF; };
inline SklnPlan skln_plan(int K, bool skinny_kf) {
  if (K % 32 == 0 && skinny_kf) return K <= 512 ? SklnPlan{2, 1, true} : K <= 1024 ? SklnPlan{4, 2, true} : SklnPlan{4, 4, true};
  return SklnPlan{gp::cdiv(K, 32) > 16 ? 4 : 2, gp::LNR_MAXC, false};
}

#endif  // SMER_GEMM_PLAN_H
