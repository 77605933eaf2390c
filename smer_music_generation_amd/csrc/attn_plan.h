// The attention dispatch of attention.hip as pure functions: which kernel
// instantiation a smer_attn_fwd / _bwd / _decode* call runs, with which grid,
// block and LDS size.  Plain C++17, no HIP and no environment: the launchers
// fill a query, read the switches their entry takes (attn_switches,
// attention.hip) and launch what the plan names; smer_attn_fwd_plan, _bwd_plan
// and _decode_plan answer the same question without launching (the mirrors
// of tests/attnref.py and tests/decoderef.py are held against them).
#ifndef SMER_ATTN_PLAN_H
#define SMER_ATTN_PLAN_H

#include <cstddef>

// thresholds and geometry the plan shares with the kernels (attention.hip
// static_asserts its own constants against these)
namespace ap {
constexpr int KVB = 64;                 // keys (or queries) per LDS tile
constexpr long TWO_GROUP_BLOCKS = 512;  // two groups per wave from this many 128-row blocks on ...
constexpr int TWO_GROUP_MAX_D = 64;     // ... and up to this head dim
constexpr long DEC_BIG_ROWS = 512;      // decode: cache capacity (key rows) of the 8-wave x 4-step forms
constexpr long DEC_PIPE_ROWS = 2048;    // ... of the pipelined key loads at any grid
constexpr long DEC_FEW_BLOCKS = 128;    // ... and the grid (rows x heads) up to which big caches pipeline too
constexpr int DEC_SHARED_G = 4;         // rows of a group per shared-memory chunk
constexpr int DEC_SPLITS = 8;           // key slices of the split entries
constexpr size_t FWD_F32_LDS_MAX = 160 * 1024;      // attn_fwd_f32: Lk * 16 bytes
constexpr size_t DEC_GENERIC_LDS_MAX = 150 * 1024;  // attn_decode_kernel: capacity * 4 bytes
inline int cdiv(long a, long b) { return (int)((a + b - 1) / b); }
}  // namespace ap

// The three values the dispatch takes from the environment, at their
// defaults; re-read on every call that uses them (tests flip them in-process).
struct AttnSwitches {
  bool f32_mfma = true;        // SMER_ATTN_F32_MFMA=0 keeps the fp32 forward on attn_fwd_f32 (A/B, tests)
  bool dec_pipe_small = true;  // SMER_DEC_PIPE_SMALL=0: grids of <= 128 blocks take the unpipelined form
  bool dec_odd_first = true;   // SMER_DECODE_ODD_FIRST=0: blocks in plain row order (A/B)
};

// two query (forward, dQ) or key (dK/dV) groups per wave once there are
// enough blocks to fill the chip
inline bool attn_two_groups(int L, int B, int H, int D) {
  return (long)ap::cdiv(L, 2 * ap::KVB) * B * H >= ap::TWO_GROUP_BLOCKS && D <= ap::TWO_GROUP_MAX_D;
}

enum AttnFamily { AF_NONE = -1, AF_BF16_FLASH, AF_F32_MFMA, AF_F32_VALU };

// a forward or backward call
struct AttnQuery {
  bool f32 = false;  // else bf16
  int B = 0, H = 0, Lq = 0, Lk = 0, D = 0;
  bool drop = false, causal = false;        // the 7-bit drop threshold is not 0
  bool mask = false, mask_in = false;       // a keep-word buffer is passed; the caller filled it (forward)
  bool q8 = false;                          // forward: the e4m3 copy of O is asked for
  bool f32_aligned = false;                 // fp32 forward: q, k 16-B aligned and ldq, ldk % 4 == 0
  bool dq_delta = true;                     // backward: the SMER_DQ_DELTA build macro
};

struct AttnFwdPlan {
  int family = AF_NONE;  // AF_NONE: bf16 with a head dim other than 32, 64, 128
  int D = 0, QG = 1;     // attn_fwd_bf16<D, QG, DROP, MIN, Q8>
  bool DROP = false, MIN = false, Q8 = false;
  int grid_x = 1, grid_y = 1, block = 256;
  size_t lds = 0;         // dynamic LDS bytes
  bool mask_gen = false;  // the mask generator runs first
};

inline AttnFwdPlan attn_fwd_plan(const AttnQuery& q, const AttnSwitches& sw) {
  AttnFwdPlan p;
  p.D = q.D; p.DROP = q.drop; p.grid_y = q.B * q.H;
  if (q.f32) {
    if (q.D == 64 && !q.drop && q.f32_aligned && sw.f32_mfma) {
      p.family = AF_F32_MFMA;
      p.grid_x = ap::cdiv(q.Lq, ap::KVB);
    } else {
      p.family = AF_F32_VALU;  // a query row per wave
      p.grid_x = ap::cdiv(q.Lq, 4);
      p.lds = (size_t)q.Lk * 16;
    }
    return p;
  }
  if (q.D != 32 && q.D != 64 && q.D != 128) return p;
  p.family = AF_BF16_FLASH;
  p.QG = attn_two_groups(q.Lq, q.B, q.H, q.D) ? 2 : 1;
  // a mask buffer: the keep words come from the generator (launched first
  // unless the caller already filled them) and the backward reads the same
  // words; no buffer: the forward hashes them itself.  With a buffer the
  // QG = 2 forward hashes the keep bits in its loop and publishes them
  // (cheaper than the separate generator: C2 encoder forward + generator
  // 125 + 29 us vs ~14x us hashing + publishing); a QG = 1 wave holds half a
  // 32-query block, so there the generator fills the buffer and the forward
  // reads it (MIN)
  p.MIN = q.drop && q.mask && (q.mask_in || p.QG == 1);
  p.mask_gen = p.MIN && !q.mask_in;
  p.Q8 = q.q8 && q.D == 64;
  p.grid_x = ap::cdiv(q.Lq, p.QG * ap::KVB);
  return p;
}

// attn_bwd_dq_bf16 / attn_bwd_dkdv_bf16<D, DROP, G, MSK, CAUSAL>
struct AttnBwdKernel {
  int D = 0, G = 1, grid_x = 1, grid_y = 1;
  bool DROP = false, MSK = false, CAUSAL = false;
};

struct AttnBwdPlan {
  int family = AF_NONE;  // AF_BF16_FLASH or AF_F32_VALU
  AttnBwdKernel dq, dkdv;
  bool dq_first = false;    // the dQ kernel forms delta = rowsum(dO * O) itself and runs first ...
  bool delta_pass = false;  // ... else a separate delta pass, then dK / dV, then dQ
  int block = 256;
  int f32_grid[4] = {0, 0, 0, 0};  // fp32: delta, P / dS, dK / dV, dQ, in launch order
};

inline AttnBwdPlan attn_bwd_plan(const AttnQuery& q, const AttnSwitches&) {
  AttnBwdPlan p;
  if (q.f32) {
    p.family = AF_F32_VALU;
    const long bh = (long)q.B * q.H;
    const long n[4] = {bh * q.Lq, bh * q.Lq * q.Lk, bh * q.Lk * q.D, bh * q.Lq * q.D};
    for (int i = 0; i < 4; ++i) p.f32_grid[i] = ap::cdiv(n[i], 256);
    return p;
  }
  p.dq_first = q.dq_delta;
  p.delta_pass = !q.dq_delta;
  if (q.D != 32 && q.D != 64 && q.D != 128) return p;
  p.family = AF_BF16_FLASH;
  // dropout variants: recompute the keep bits by hashing, or read the
  // forward's stored bits (MSK); causal and non-causal instances
  auto kernel = [&](int L) {
    AttnBwdKernel k;
    k.D = q.D; k.G = attn_two_groups(L, q.B, q.H, q.D) ? 2 : 1;
    k.DROP = q.drop; k.MSK = q.drop && q.mask; k.CAUSAL = q.causal;
    k.grid_x = ap::cdiv(L, k.G * ap::KVB); k.grid_y = q.B * q.H;
    return k;
  };
  p.dq = kernel(q.Lq);
  p.dkdv = kernel(q.Lk);
  return p;
}

enum DecEntry { DE_DECODE, DE_QLN, DE_SHARED, DE_SHARED_QLN, DE_SPLIT_F32, DE_SPLIT_QLN_F32, DE_COUNT };
enum DecKind { DK_GENERIC, DK_VEC, DK_SHARED };

struct DecQuery {
  int entry = DE_DECODE;
  bool f32 = false;  // else bf16
  int D = 0, n_rows = 0, H = 0, n_groups = 0, dmodel = 0;
  long row_stride = 0, req_stride = 0, head_stride = 0;
  bool vec_ok = false;  // smer_attn_decode: q, caches, o 16-B aligned, every stride a multiple of 16 B
};

// attn_decode_kernel<T> (generic), attn_decode_vec_kernel<T, LPK, UNR, NW,
// PIPE, QP, NS> (vec) or attn_decode_shared_kernel<LPK, UNR, NW, PIPE, QP, G>
struct DecPlan {
  int kind = DK_GENERIC, LPK = 0, UNR = 0, NW = 0, QP = 0, NS = 0;
  bool f32 = false, PIPE = false;
  int grid_x = 1, grid_y = 1, grid_z = 1, block = 256;
  size_t lds = 0;
  int odd = 0;   // odd rows first (the kernel's odd_first argument)
  long cap = 0;  // key capacity of a request
};

// key capacity of a request in cache rows (heads side by side within a key
// row: head_stride == D)
inline long dec_cap_rows(long row_stride, long req_stride, long head_stride, int D) {
  return (head_stride != D ? head_stride : req_stride) / (row_stride > 0 ? row_stride : 1);
}

inline DecPlan attn_decode_plan(const DecQuery& q, const AttnSwitches& sw) {
  DecPlan p;
  p.f32 = q.f32;
  p.cap = dec_cap_rows(q.row_stride, q.req_stride, q.head_stride > 0 ? q.head_stride : q.D, q.D);
  p.grid_x = q.H; p.grid_y = q.n_rows;  // the H blocks of a row read the same K/V rows together
  if (q.entry == DE_SPLIT_F32 || q.entry == DE_SPLIT_QLN_F32) {
    // fp32 over DEC_SPLITS key slices per (row, head).  Pipelined key loads
    // (the next key step requested before this step's math; the same
    // arithmetic as the unpipelined form, so the same bits): batch-1 plugin
    // call 2,621 vs 2,534 tokens/s (two rounds, tools/batch1_bench.py env
    // SMER_DEC_SPLIT_CFG; 8-wave and 4-step forms 2,558-2,607)
    p.kind = DK_VEC; p.f32 = true;
    p.LPK = 16; p.UNR = 2; p.NW = 4; p.PIPE = true; p.QP = q.dmodel; p.NS = ap::DEC_SPLITS;
    p.grid_z = ap::DEC_SPLITS;
    return p;
  }
  const bool qln = q.entry == DE_QLN || q.entry == DE_SHARED_QLN;
  // vectorised path: 16-B aligned rows, LPK = D / (16 / elem) in {4, 8, 16};
  // else attn_decode_kernel: a block per (row, head), the scores in LDS
  const int vec = q.f32 ? 4 : 8, lpk = q.D / vec;
  if (q.entry == DE_DECODE && !(q.vec_ok && q.D % vec == 0 && (lpk == 4 || lpk == 8 || lpk == 16))) {
    p.grid_x = q.n_rows; p.grid_y = q.H;
    p.lds = (size_t)p.cap * sizeof(float);
    return p;
  }
  // long memories get 8 waves x 4 steps of loads in flight per block, short
  // self-attention caches 4 x 2 (the query-prologue entries: always 8 x 4)
  const bool big = qln || p.cap >= ap::DEC_BIG_ROWS;
  // the next key step's loads issued before the current step's math: long
  // memories, and big ones with few blocks (the batch-1 plugin step: 16
  // blocks stream a ~1k-key memory each; the same arithmetic as the
  // unpipelined 8-wave form, so the logits do not depend on the batch).
  // The query-prologue entries leave the few-blocks term out
  p.PIPE = p.cap >= ap::DEC_PIPE_ROWS || (!qln && big && (long)q.n_rows * q.H <= ap::DEC_FEW_BLOCKS && sw.dec_pipe_small);
  p.LPK = lpk; p.UNR = big ? 4 : 2; p.NW = big ? 8 : 4;
  p.block = 64 * p.NW;
  p.QP = qln ? q.dmodel : 0;
  if (q.entry == DE_SHARED || q.entry == DE_SHARED_QLN) {
    // every group has at most one partial chunk, so n_rows / G + n_groups
    // chunks bound any split
    p.kind = DK_SHARED;
    p.grid_y = q.n_rows / ap::DEC_SHARED_G + q.n_groups;
    return p;
  }
  p.kind = DK_VEC;
  p.odd = sw.dec_odd_first;
  return p;
}

#endif  // SMER_ATTN_PLAN_H
