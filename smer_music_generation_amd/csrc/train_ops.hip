// Training-step tail: the fused multi-criterion weighted cross entropy
// (train.py:555-642, 726-780), torch.optim.Adam (train.py:264, 786), bias
// gradient column sums and dtype casts.  All HBM-bound elementwise / row
// kernels; reductions are fixed-order (bitwise reproducible).
#include "common.h"

// denom = sum_i ce_all[y_i]   (single workgroup, fixed order)
__global__ __launch_bounds__(256) void wce_denom_kernel(int n, const int64_t* __restrict__ y,
                                                        const float* __restrict__ ce_all,
                                                        float* __restrict__ denom) {
  __shared__ float red[256];
  float a = 0.f;
  for (int i = threadIdx.x; i < n; i += 256) a += ce_all[y[i]];
  red[threadIdx.x] = a;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) *denom = red[0];
}

template <typename T>
__global__ __launch_bounds__(256) void wce_kernel(int R, int V, const float* __restrict__ logits,
                                                  long ldl, const int64_t* __restrict__ y,
                                                  const float* __restrict__ w,
                                                  const float* __restrict__ denom,
                                                  float* __restrict__ row_loss,
                                                  T* __restrict__ dlog, long ldd,
                                                  float grad_scale) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= R) return;
  const float* x = logits + (long)r * ldl;
  const long yt = y[r];
  float mx = -INFINITY;
  for (int v = lane; v < V; v += 64) mx = fmaxf(mx, x[v]);
  mx = wave_max(mx);
  float se = 0.f;
  for (int v = lane; v < V; v += 64) se += expf(x[v] - mx);
  se = wave_sum(se);
  const float wy = yt == 0 ? 0.f : w[yt];
  // -log_softmax(x)[y] = log(se) - (x[y] - mx): both terms are of the loss's
  // own size (mx + log(se) - x[y] cancels at the logits' magnitude)
  if (lane == 0) row_loss[r] = wy * (logf(se) - (x[yt] - mx));
  if (dlog) {
    const float coef = grad_scale * wy / *denom;
    const float inv = 1.f / se;
    for (int v = lane; v < V; v += 64) {
      float g = coef * (expf(x[v] - mx) * inv - (v == yt ? 1.f : 0.f));
      dlog[(long)r * ldd + v] = from_f32<T>(g);
    }
  }
}

// smer_wce_fwd_bwd_ex: wce_kernel with torch's label_smoothing = ls on the
// twelve criteria, and the plain term w[y] * -log_softmax(x)[y] beside the
// row loss (row_nll, nullable).  Same layout: one wave per row, four rows per
// workgroup, fixed-order wave reductions.  LS = false is wce_kernel's own
// code, expression for expression (ls = 0 gives its bits).  LS = true, on a
// row with y != 0 (an ignored row gets no smoothing term):
//   row_loss = (1-ls) * nll + (ls/V) * sum_c w[c] * -log_softmax(x)[c]
//   dlog[c]  = grad_scale/denom * ((1-ls) * w[y] * (p[c] - [c == y])
//                                  + (ls/V) * (W * p[c] - w[c])),  W = sum_c w[c]
// Each -log_softmax(x)[c] = log(se) - (x[c] - mx) is a sum of two
// non-negative terms, as in the plain loss (W * lse - sum w x would cancel at
// the logits' magnitude).  W is summed by every wave in the same order, so
// every row sees the same bits.  x[c] = -inf gives w[c] * inf in the sum, as
// torch does: inf for w[c] > 0 (NaN for w[c] == 0), in that row alone.
template <typename T, bool LS>
__global__ __launch_bounds__(256) void wce_ex_kernel(int R, int V, const float* __restrict__ logits,
                                                     long ldl, const int64_t* __restrict__ y,
                                                     const float* __restrict__ w,
                                                     const float* __restrict__ denom,
                                                     float* __restrict__ row_loss,
                                                     float* __restrict__ row_nll,
                                                     T* __restrict__ dlog, long ldd,
                                                     float grad_scale, float ls) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= R) return;
  const float* x = logits + (long)r * ldl;
  const long yt = y[r];
  float mx = -INFINITY;
  for (int v = lane; v < V; v += 64) mx = fmaxf(mx, x[v]);
  mx = wave_max(mx);
  float se = 0.f;
  for (int v = lane; v < V; v += 64) se += expf(x[v] - mx);
  se = wave_sum(se);
  const float wy = yt == 0 ? 0.f : w[yt];
  const float nll = wy * (logf(se) - (x[yt] - mx));
  if constexpr (!LS) {
    if (lane == 0) {
      row_loss[r] = nll;
      if (row_nll) row_nll[r] = nll;
    }
    if (dlog) {
      const float coef = grad_scale * wy / *denom;
      const float inv = 1.f / se;
      for (int v = lane; v < V; v += 64) {
        float g = coef * (expf(x[v] - mx) * inv - (v == yt ? 1.f : 0.f));
        dlog[(long)r * ldd + v] = from_f32<T>(g);
      }
    }
  } else {
    const bool live = yt != 0;
    const float lse = logf(se);
    float W = 0.f, sm = 0.f;
    for (int v = lane; v < V; v += 64) {
      const float wv = w[v];
      W += wv;
      sm += wv * (lse - (x[v] - mx));
    }
    W = wave_sum(W);
    sm = wave_sum(sm);
    const float uni = ls / (float)V;
    if (lane == 0) {
      row_loss[r] = live ? (1.f - ls) * nll + uni * sm : 0.f;
      if (row_nll) row_nll[r] = nll;
    }
    if (dlog) {
      const float cy = grad_scale * (1.f - ls) * wy / *denom;
      const float cu = live ? grad_scale * uni / *denom : 0.f;
      const float inv = 1.f / se;
      for (int v = lane; v < V; v += 64) {
        const float p = expf(x[v] - mx) * inv;
        float g = cy * (p - (v == yt ? 1.f : 0.f)) + cu * (W * p - w[v]);
        dlog[(long)r * ldd + v] = from_f32<T>(g);
      }
    }
  }
}

__global__ __launch_bounds__(256) void sum_div_kernel(int n, const float* __restrict__ x,
                                                      const float* __restrict__ denom,
                                                      float* __restrict__ out) {
  __shared__ float red[256];
  float a = 0.f;
  for (int i = threadIdx.x; i < n; i += 256) a += x[i];
  red[threadIdx.x] = a;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) *out = denom ? red[0] / *denom : red[0];
}

// torch.optim.Adam (_single_tensor_adam): m.lerp_(g, 1-b1); v = b2 v + (1-b2) g^2;
// p -= (lr/bc1) * m / (sqrt(v)/sqrt(bc2) + eps)
//
// One templated kernel, two instantiations: the unguarded one takes
// smer_adam's arguments and compiles to the code it always had.  GUARDED (smer_adam_guarded) reads the control block
// of smer_clip_scale: ctl[2] != 0 (non-finite gradient norm) leaves every
// buffer untouched, otherwise the update runs on fl32(g * ctl[1]).  The
// product passes through an empty value barrier: without it hipcc contracts
// the multiply into the g - m subtraction (v_fma_f32 s, g, -m) and
// re-associates the v update, and the result is no longer smer_adam's on the
// rounded product.  With it the two instantiations differ by the skip test
// and one v_mul_f32 (tests/test_gradclip_gpu.py holds them bit-equal).
__device__ __forceinline__ const float* adam_ctl(const float* ctl) { return ctl; }
template <bool GUARDED, typename... CTL>  // CTL: (const float*) when GUARDED, else empty
__global__ void adam_kernel(long n, float* __restrict__ p, const float* __restrict__ g,
                            float* __restrict__ m, float* __restrict__ v, bf16* __restrict__ pb,
                            float lr, float b1, float b2, float eps, float bc1, float bc2s, CTL... ctl) {
  static_assert(sizeof...(CTL) == (GUARDED ? 1 : 0), "the control block goes with the guarded kernel");
  float gs = 1.f;
  if constexpr (GUARDED) {
    const float* __restrict__ c = adam_ctl(ctl...);
    if (c[2] != 0.f) return;
    gs = c[1];
  }
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long stride = (long)gridDim.x * blockDim.x;
  const float step = lr / bc1;
  for (; i < n; i += stride) {
    float gi = g[i];
    if constexpr (GUARDED) {
      gi = gi * gs;
      asm volatile("" : "+v"(gi));
    }
    float mi = m[i];
    mi = mi + (1.f - b1) * (gi - mi);
    float vi = v[i] * b2 + (1.f - b2) * gi * gi;
    float den = sqrtf(vi) / bc2s + eps;
    float pi = p[i] - step * (mi / den);
    m[i] = mi;
    v[i] = vi;
    p[i] = pi;
    if (pb) pb[i] = (bf16)pi;
  }
}

// smer_adam_ex: the step above with weight decay and an exponential moving
// average of the weights in the same pass.  Per element, in adam_kernel's own
// arithmetic: gi = fl(g * ctl[1]) when GUARDED; WD == 1 (coupled L2, torch
// Adam(weight_decay=)): gi += wd * p, after the clip scale; WD == 2
// (decoupled, torch AdamW): p *= decay_mul before the update; EMA: e += (1 -
// ema_decay) * (p_new - e).  The value barriers keep gi, the decayed weight
// and the stored weight the rounded values they are documented to be (see
// adam_kernel), so WD == 0 without EMA is adam_kernel bit for bit
// (tests/test_adam_ex_gpu.py).
struct AdamExArgs {
  float lr, b1, b2, eps, bc1, bc2s, wd, decay_mul, ema_decay;
};

template <bool GUARDED, int WD, bool EMA>
__device__ __forceinline__ void adam_ex_elem(const AdamExArgs& a, float step, float gs, float& p, float g,
                                             float& m, float& v, float& e) {
  float gi = g;
  if constexpr (GUARDED) {
    gi = gi * gs;
    asm volatile("" : "+v"(gi));
  }
  float pi = p;
  if constexpr (WD == 1) {
    gi = __builtin_fmaf(a.wd, pi, gi);
    asm volatile("" : "+v"(gi));
  }
  if constexpr (WD == 2) {
    pi = pi * a.decay_mul;
    asm volatile("" : "+v"(pi));
  }
  // adam_kernel's expressions with the contractions written out as hipcc
  // forms them there (which product of v * b2 + (1 - b2) * g * g it fuses
  // depends on the loop around it: left alone, this kernel's scalar loop
  // fused the other one and lost the last bit of v)
  float mi = m;
  mi = __builtin_fmaf(1.f - a.b1, gi - mi, mi);
  float vi = __builtin_fmaf((1.f - a.b2) * gi, gi, v * a.b2);
  float den = sqrtf(vi) / a.bc2s + a.eps;
  pi = __builtin_fmaf(-step, mi / den, pi);
  m = mi;
  v = vi;
  p = pi;
  if constexpr (EMA) {
    asm volatile("" : "+v"(pi));
    e = __builtin_fmaf(1.f - a.ema_decay, pi - e, e);
  }
}

// Elements [head, head + 4 nvec) go as 16-B vectors of p/g/m/v/ema and 8-B
// vectors of the bf16 copy (the host picks head so that all of them are
// aligned there, or head = n when the bases disagree); the n - 4 nvec
// elements in front of and behind them go one by one.  Every element is
// updated by exactly one lane from its own inputs: no atomics, no workspace,
// and a range split into several launches gets the same bits.
template <bool GUARDED, int WD, bool EMA>
__global__ __launch_bounds__(256) void adam_ex_kernel(long n, long head, long nvec, float* __restrict__ p,
                                                      const float* __restrict__ g, float* __restrict__ m,
                                                      float* __restrict__ v, bf16* __restrict__ pb,
                                                      float* __restrict__ ema, const float* __restrict__ ctl,
                                                      AdamExArgs a) {
  float gs = 1.f;
  if constexpr (GUARDED) {
    if (ctl[2] != 0.f) return;
    gs = ctl[1];
  }
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  const long stride = (long)gridDim.x * 256;
  const float step = a.lr / a.bc1;
  for (long k = t; k < nvec; k += stride) {
    const long i = head + 4 * k;
    f32x4 P = *reinterpret_cast<const f32x4*>(p + i);
    const f32x4 G = *reinterpret_cast<const f32x4*>(g + i);
    f32x4 M = *reinterpret_cast<const f32x4*>(m + i);
    f32x4 V = *reinterpret_cast<const f32x4*>(v + i);
    f32x4 E = {0.f, 0.f, 0.f, 0.f};
    if constexpr (EMA) E = *reinterpret_cast<const f32x4*>(ema + i);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float pj = P[j], mj = M[j], vj = V[j], ej = E[j];
      adam_ex_elem<GUARDED, WD, EMA>(a, step, gs, pj, G[j], mj, vj, ej);
      P[j] = pj, M[j] = mj, V[j] = vj, E[j] = ej;
    }
    *reinterpret_cast<f32x4*>(m + i) = M;
    *reinterpret_cast<f32x4*>(v + i) = V;
    *reinterpret_cast<f32x4*>(p + i) = P;
    if (pb) {
      bf16x4 B;
#pragma unroll
      for (int j = 0; j < 4; ++j) B[j] = (bf16)P[j];
      *reinterpret_cast<bf16x4*>(pb + i) = B;
    }
    if constexpr (EMA) *reinterpret_cast<f32x4*>(ema + i) = E;
  }
  const long nscalar = n - 4 * nvec;
  for (long s = t; s < nscalar; s += stride) {
    const long i = s < head ? s : s + 4 * nvec;
    float pi = p[i], mi = m[i], vi = v[i], ei = 0.f;
    if constexpr (EMA) ei = ema[i];
    adam_ex_elem<GUARDED, WD, EMA>(a, step, gs, pi, g[i], mi, vi, ei);
    m[i] = mi;
    v[i] = vi;
    p[i] = pi;
    if (pb) pb[i] = (bf16)pi;
    if constexpr (EMA) ema[i] = ei;
  }
}

// smer_adam_groups: smer_adam_ex with the hyper-parameters of a parameter
// group per element.  Group membership is constant on 64-element blocks (a
// parameter's slot is 64-aligned), gmap holds one byte per block of the flat
// buffer and block0 is the block of this slice's first element.  The table
// travels by value in the kernel arguments.
//
// A lane owns one 16-B vector, so 16 lanes share a block and a wave iteration
// covers four.  The wave runs a waterfall over the group ids its lanes hold:
// readfirstlane picks one, the lanes that hold it update their vector through
// adam_ex_elem with that group's row -- read from the kernel arguments with a
// wave-uniform index, so it stays in scalar registers, never scratch -- and
// the loop ends when no lane is left: one pass wherever a wave sees one group,
// four at most.  The arithmetic is adam_ex_elem's and nothing else, so an
// element of group k gets the bits smer_adam_ex writes with k's arguments
// (tests/test_param_groups_gpu.py).  n % 64 == 0 and 16-B aligned bases (8-B
// for the bf16 copy): there is no scalar head or tail.  One lane per element,
// no atomics, no workspace; a range split at a block boundary gets the same
// bits.
struct AdamGroupTable {
  smer_adam_group row[SMER_ADAM_MAX_GROUPS];
};

template <bool GUARDED, int WD, bool EMA>
__device__ __forceinline__ void adam_groups_vec(const AdamExArgs& a, float gs, f32x4& P, const f32x4& G,
                                                f32x4& M, f32x4& V, f32x4& E) {
  const float step = a.lr / a.bc1;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    float pj = P[j], mj = M[j], vj = V[j], ej = E[j];
    adam_ex_elem<GUARDED, WD, EMA>(a, step, gs, pj, G[j], mj, vj, ej);
    P[j] = pj, M[j] = mj, V[j] = vj, E[j] = ej;
  }
}

template <bool GUARDED, bool EMA>
__global__ __launch_bounds__(256) void adam_groups_kernel(long nvec, float* __restrict__ p,
                                                          const float* __restrict__ g, float* __restrict__ m,
                                                          float* __restrict__ v, bf16* __restrict__ pb,
                                                          float* __restrict__ ema, const float* __restrict__ ctl,
                                                          const uint8_t* __restrict__ gmap, long block0,
                                                          float ema_decay, AdamGroupTable tab) {
  float gs = 1.f;
  if constexpr (GUARDED) {
    if (ctl[2] != 0.f) return;
    gs = ctl[1];
  }
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  const long stride = (long)gridDim.x * 256;
  for (long k = t; k < nvec; k += stride) {
    const long i = 4 * k;
    const int gid = gmap[block0 + (k >> 4)];
    f32x4 P = *reinterpret_cast<const f32x4*>(p + i);
    const f32x4 G = *reinterpret_cast<const f32x4*>(g + i);
    f32x4 M = *reinterpret_cast<const f32x4*>(m + i);
    f32x4 V = *reinterpret_cast<const f32x4*>(v + i);
    f32x4 E = {0.f, 0.f, 0.f, 0.f};
    if constexpr (EMA) E = *reinterpret_cast<const f32x4*>(ema + i);
    bool todo = true;
    while (todo) {
      const int cur = __builtin_amdgcn_readfirstlane(gid);
      // the table index as a scalar the compiler cannot equate with gid: under
      // gid == cur it would index with the per-lane gid instead (vector loads
      // of the row).  The mask keeps the read inside the table whatever the
      // map holds.
      int row = cur & (SMER_ADAM_MAX_GROUPS - 1);
      asm volatile("" : "+s"(row));
      if (gid == cur) {
        const smer_adam_group& r = tab.row[row];
        const AdamExArgs a{r.lr, r.b1, r.b2, r.eps, r.bc1, r.bc2_sqrt, r.wd, r.decay_mul, ema_decay};
        if (r.wd_mode == 0) adam_groups_vec<GUARDED, 0, EMA>(a, gs, P, G, M, V, E);
        else if (r.wd_mode == 1) adam_groups_vec<GUARDED, 1, EMA>(a, gs, P, G, M, V, E);
        else adam_groups_vec<GUARDED, 2, EMA>(a, gs, P, G, M, V, E);
        todo = false;
      }
    }
    *reinterpret_cast<f32x4*>(m + i) = M;
    *reinterpret_cast<f32x4*>(v + i) = V;
    *reinterpret_cast<f32x4*>(p + i) = P;
    if (pb) {
      bf16x4 B;
#pragma unroll
      for (int j = 0; j < 4; ++j) B[j] = (bf16)P[j];
      *reinterpret_cast<bf16x4*>(pb + i) = B;
    }
    if constexpr (EMA) *reinterpret_cast<f32x4*>(ema + i) = E;
  }
}

// Global gradient norm, stage 1: part[c] = sum of squares of chunk c
// (GN_CH floats) of a range.  256 lanes x 4 iterations x 4 independent 16-B
// loads; lane accumulator u takes load u of every iteration (16 fmas in
// element order), then (a0 + a1) + (a2 + a3), the wave butterfly and
// (w0 + w1) + (w2 + w3): the order is fixed by the element's position in
// its chunk alone, so a partial is a pure function of the chunk's contents.
// Elements at or behind n are never read (they add an exact +0).
constexpr int GN_CH = 16384;
constexpr int GN_IT = 4, GN_U = 4;
static_assert(GN_CH == GN_IT * GN_U * 256 * 4, "chunk = iterations x loads x lanes x 4 floats");
__global__ __launch_bounds__(256) void grad_sqnorm_kernel(long n, const float* __restrict__ g,
                                                          float* __restrict__ part) {
  __shared__ float red[4];
  const long base = (long)blockIdx.x * GN_CH;
  const long rem = n - base;
  const int cnt = rem < (long)GN_CH ? (int)rem : GN_CH;
  const float* __restrict__ p = g + base;
  float a[GN_U] = {0.f, 0.f, 0.f, 0.f};
  if (cnt == GN_CH) {
#pragma unroll
    for (int it = 0; it < GN_IT; ++it) {
      float4 x[GN_U];
#pragma unroll
      for (int u = 0; u < GN_U; ++u)
        x[u] = *reinterpret_cast<const float4*>(p + ((it * GN_U + u) * 256 + (int)threadIdx.x) * 4);
#pragma unroll
      for (int u = 0; u < GN_U; ++u) {
        a[u] = __builtin_fmaf(x[u].x, x[u].x, a[u]);
        a[u] = __builtin_fmaf(x[u].y, x[u].y, a[u]);
        a[u] = __builtin_fmaf(x[u].z, x[u].z, a[u]);
        a[u] = __builtin_fmaf(x[u].w, x[u].w, a[u]);
      }
    }
  } else {
    for (int it = 0; it < GN_IT; ++it) {
#pragma unroll
      for (int u = 0; u < GN_U; ++u) {
        const int e = ((it * GN_U + u) * 256 + (int)threadIdx.x) * 4;
        float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
        if (e + 4 <= cnt) {
          x = *reinterpret_cast<const float4*>(p + e);
        } else if (e < cnt) {
          x.x = p[e];
          if (e + 1 < cnt) x.y = p[e + 1];
          if (e + 2 < cnt) x.z = p[e + 2];
        }
        a[u] = __builtin_fmaf(x.x, x.x, a[u]);
        a[u] = __builtin_fmaf(x.y, x.y, a[u]);
        a[u] = __builtin_fmaf(x.z, x.z, a[u]);
        a[u] = __builtin_fmaf(x.w, x.w, a[u]);
      }
    }
  }
  float s = wave_sum((a[0] + a[1]) + (a[2] + a[3]));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// Stage 2, one workgroup: the partials summed in double (lane t takes
// t, t + 256, .. in index order, then a fixed tree), norm = fl32(sqrt),
// scale = min(1, max_norm / (norm + 1e-6)) in fp32 the way
// torch.nn.utils.clip_grad_norm_ evaluates it (scalar / tensor is
// tensor.reciprocal() * scalar: two roundings), the skip flag and the count.
__global__ __launch_bounds__(256) void clip_scale_kernel(int nparts, const float* __restrict__ part,
                                                         float max_norm, float* __restrict__ ctl) {
  __shared__ double red[256];
  double a = 0.0;
  for (int i = threadIdx.x; i < nparts; i += 256) a += (double)part[i];
  red[threadIdx.x] = a;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const float norm = (float)sqrt(red[0]);
    const bool finite = fabsf(norm) <= 3.402823466e+38f;  // false for inf and NaN
    const float skip = finite ? 0.f : 1.f;
    ctl[0] = norm;
    ctl[1] = finite ? fminf(1.f, smer_div_rn(1.f, norm + 1e-6f) * max_norm) : 0.f;
    ctl[2] = skip;
    ctl[3] += skip;
  }
}

template <typename S, typename D>
__global__ void cast_kernel(long n, const S* __restrict__ s, D* __restrict__ d) {
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long stride = (long)gridDim.x * blockDim.x;
  for (; i < n; i += stride) d[i] = from_f32<D>(to_f32(s[i]));
}

// Stage 1: workgroup = 512 columns (64 lanes x 8 via 16-B loads) x CS_ROWS
// rows (4 row groups, 4 independent loads in flight each); fixed-order
// combine of the 4 groups -> part[rowblock][N].
constexpr int CS_ROWS = 64;
template <typename T, bool VEC>
__global__ __launch_bounds__(256) void colsum_part_kernel(int M, int N, const T* __restrict__ x,
                                                          long ldx, float* __restrict__ part) {
  __shared__ float red[4][512];
  const int cg = threadIdx.x & 63, rg = threadIdx.x >> 6;
  const int c0 = blockIdx.x * 512 + cg * 8;
  const int r0 = blockIdx.y * CS_ROWS;
  const int r1 = min(M, r0 + CS_ROWS);
  const int valid = min(8, N - c0);
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (valid > 0) {
    int r = r0 + rg;
    for (; r + 12 < r1; r += 16) {
      float v0[8], v1[8], v2[8], v3[8];
      load8<T, VEC>(x + (long)r * ldx + c0, valid, v0);
      load8<T, VEC>(x + (long)(r + 4) * ldx + c0, valid, v1);
      load8<T, VEC>(x + (long)(r + 8) * ldx + c0, valid, v2);
      load8<T, VEC>(x + (long)(r + 12) * ldx + c0, valid, v3);
#pragma unroll
      for (int i = 0; i < 8; ++i) acc[i] += (v0[i] + v1[i]) + (v2[i] + v3[i]);
    }
    for (; r < r1; r += 4) {
      float v0[8];
      load8<T, VEC>(x + (long)r * ldx + c0, valid, v0);
#pragma unroll
      for (int i = 0; i < 8; ++i) acc[i] += v0[i];
    }
  }
#pragma unroll
  for (int i = 0; i < 8; ++i) red[rg][cg * 8 + i] = acc[i];
  __syncthreads();
  for (int c = threadIdx.x; c < 512; c += 256) {
    int col = blockIdx.x * 512 + c;
    if (col < N) part[(long)blockIdx.y * N + col] = (red[0][c] + red[1][c]) + (red[2][c] + red[3][c]);
  }
}

// Workgroup (x = 64-column tile, y = chunk of `chunk` partial rows) writes
// out[y * ostride + col] (columns >= nsplit go to out2[col - nsplit]); rows
// summed in a fixed order (deterministic).
__global__ void __launch_bounds__(256) smer_col_reduce(int nblk, int N, const float* __restrict__ part,
                                                       long stride, long off, float* __restrict__ out,
                                                       long ostride, int chunk, int accumulate,
                                                       float scale, float* __restrict__ out2,
                                                       int nsplit) {
  __shared__ float red[4][64];
  const int cl = threadIdx.x & 63, g = threadIdx.x >> 6;
  const int col = blockIdx.x * 64 + cl;
  const int b0 = blockIdx.y * chunk, b1 = min(nblk, b0 + chunk);
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
  if (col < N) {
    const float* p = part + off + col;
    int b = b0 + g;
    for (; b + 12 < b1; b += 16) {
      a0 += p[(long)b * stride];
      a1 += p[(long)(b + 4) * stride];
      a2 += p[(long)(b + 8) * stride];
      a3 += p[(long)(b + 12) * stride];
    }
    for (; b < b1; b += 4) a0 += p[(long)b * stride];
  }
  red[g][cl] = (a0 + a1) + (a2 + a3);
  __syncthreads();
  if (g == 0 && col < N) {
    float a = ((red[0][cl] + red[1][cl]) + (red[2][cl] + red[3][cl])) * scale;
    float* o = col < nsplit ? out + (long)blockIdx.y * ostride + col
                            : out2 + (long)blockIdx.y * ostride + (col - nsplit);
    *o = accumulate ? *o + a : a;
  }
}

size_t smer_col_reduce_scratch(int nblk, int N) {
  return nblk > 64 ? (size_t)((nblk + 63) / 64) * N * sizeof(float) : 0;
}

void smer_col_reduce_launch(int nblk, int N, const float* part, long stride, long off, float* out,
                            int accumulate, float scale, float* scratch, hipStream_t s,
                            float* out2, int nsplit) {
  dim3 gx((N + 63) / 64);
  if (!out2) nsplit = N;
  if (nblk > 64) {
    int g = (nblk + 63) / 64;
    hipLaunchKernelGGL(smer_col_reduce, dim3(gx.x, g), dim3(256), 0, s, nblk, N, part, stride,
                       off, scratch, (long)N, 64, 0, 1.f, (float*)nullptr, N);
    hipLaunchKernelGGL(smer_col_reduce, dim3(gx.x, 1), dim3(256), 0, s, g, N,
                       (const float*)scratch, (long)N, 0L, out, 0L, g, accumulate, scale, out2,
                       nsplit);
  } else {
    hipLaunchKernelGGL(smer_col_reduce, dim3(gx.x, 1), dim3(256), 0, s, nblk, N, part, stride,
                       off, out, 0L, nblk, accumulate, scale, out2, nsplit);
  }
}

// Rows [b0, b1) of one column as row group g of smer_col_reduce sums them:
// four round-robin accumulators over rows g, g + 4, ..., then the pair sums.
__device__ __forceinline__ float col_reduce_group(const float* p, long stride, int b0, int b1, int g) {
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
  int b = b0 + g;
  for (; b + 12 < b1; b += 16) {
    a0 += p[(long)b * stride];
    a1 += p[(long)(b + 4) * stride];
    a2 += p[(long)(b + 8) * stride];
    a3 += p[(long)(b + 12) * stride];
  }
  for (; b < b1; b += 4) a0 += p[(long)b * stride];
  return (a0 + a1) + (a2 + a3);
}

// All of a step's LayerNorm dgamma / dbeta reductions in one launch:
// workgroup (x = 64-column tile, y = site) does for its columns what
// smer_col_reduce_launch does in one or two launches, operation for
// operation (same accumulators, same pair sums, the 64-row chunk sums kept
// in LDS where the two launches pass them through scratch), so the sums are
// bit for bit the per-call ones.  A full chunk's 16 rows per thread are
// loaded ahead, one chunk in front of the adds: the reduction is a stream
// of 256-B row segments and would otherwise wait a round trip per row.
__global__ void __launch_bounds__(256) smer_ln_param_reduce_batch(const smer_ln_reduce_site* __restrict__ sites) {
  __shared__ float red[2][4][64];
  __shared__ float csum[SMER_LN_REDUCE_MAX_NBLK / 64][64];
  const smer_ln_reduce_site st = sites[blockIdx.y];
  const int cl = threadIdx.x & 63, g = threadIdx.x >> 6;
  const int nblk = st.nblk, N = st.N;
  const bool both = st.dgamma && st.dbeta;
  const int ncol = both ? 2 * N : N;  // reduced width: dgamma | dbeta, or one of them
  if ((int)blockIdx.x * 64 >= ncol || (!st.dgamma && !st.dbeta) || nblk <= 0 ||
      nblk > SMER_LN_REDUCE_MAX_NBLK)
    return;  // uniform over the workgroup
  const long stride = 2L * N;
  const int col = blockIdx.x * 64 + cl;
  const bool live = col < ncol;
  const float* p = st.part + (st.dgamma ? 0 : N) + (live ? col : 0);
  float* out = st.dgamma ? st.dgamma : st.dbeta;
  const int nsplit = both ? N : ncol;
  float total;
  if (nblk <= 64) {
    red[0][g][cl] = live ? col_reduce_group(p, stride, 0, nblk, g) : 0.f;
    __syncthreads();
    total = (red[0][0][cl] + red[0][1][cl]) + (red[0][2][cl] + red[0][3][cl]);
  } else {
    const int nch = (nblk + 63) / 64, nfull = nblk / 64;
    float v[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) v[i] = live ? p[(long)(g + 4 * i) * stride] : 0.f;
    for (int c = 0; c < nfull; ++c) {
      float w[16];
      if (c + 1 < nfull) {
#pragma unroll
        for (int i = 0; i < 16; ++i) w[i] = live ? p[(long)((c + 1) * 64 + g + 4 * i) * stride] : 0.f;
      }
      float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        a0 += v[4 * k];
        a1 += v[4 * k + 1];
        a2 += v[4 * k + 2];
        a3 += v[4 * k + 3];
      }
      // red is double-buffered: chunk c + 1 writes the other half while row
      // group 0 may still read this one; chunk c + 2 comes after c + 1's barrier
      red[c & 1][g][cl] = (a0 + a1) + (a2 + a3);
      __syncthreads();
      if (g == 0)
        csum[c][cl] = (red[c & 1][0][cl] + red[c & 1][1][cl]) + (red[c & 1][2][cl] + red[c & 1][3][cl]);
      if (c + 1 < nfull) {
#pragma unroll
        for (int i = 0; i < 16; ++i) v[i] = w[i];
      }
    }
    if (nch > nfull) {  // ragged last chunk
      const int c = nfull;
      red[c & 1][g][cl] = live ? col_reduce_group(p, stride, c * 64, nblk, g) : 0.f;
      __syncthreads();
      if (g == 0)
        csum[c][cl] = (red[c & 1][0][cl] + red[c & 1][1][cl]) + (red[c & 1][2][cl] + red[c & 1][3][cl]);
    }
    __syncthreads();
    // the second launch's pattern over the nch chunk sums
    const float r = col_reduce_group(&csum[0][cl], 64, 0, nch, g);
    red[0][g][cl] = r;
    __syncthreads();
    total = (red[0][0][cl] + red[0][1][cl]) + (red[0][2][cl] + red[0][3][cl]);
  }
  if (g == 0 && live) {
    float* o = col < nsplit ? out + col : st.dbeta + (col - nsplit);
    *o = st.accumulate ? *o + total : total;
  }
}

void smer_ln_param_reduce_batch_launch(int nsites, int max_cols, const smer_ln_reduce_site* sites_dev,
                                       hipStream_t s) {
  if (nsites <= 0 || max_cols <= 0) return;
  hipLaunchKernelGGL(smer_ln_param_reduce_batch, dim3((max_cols + 63) / 64, nsites), dim3(256), 0, s,
                     sites_dev);
}

// ---------------------------------------------------------------------------
extern "C" int smer_wce_denom(int n, const int64_t* y, const float* ce_all, float* denom,
                              smer_stream_t stream) {
  SMER_REQUIRE(y && ce_all && denom, "smer_wce_denom: null pointer");
  hipLaunchKernelGGL(wce_denom_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, n, y, ce_all,
                     denom);
  SMER_CHECK_LAUNCH("smer_wce_denom");
  return SMER_OK;
}

extern "C" int smer_wce_fwd_bwd(int dtype, int R, int V, const float* logits, long ldl,
                                const int64_t* y, const float* w, const float* denom,
                                float* row_loss, float* loss_out, void* dlogits, long ldd,
                                float grad_scale, smer_stream_t stream) {
  SMER_REQUIRE(logits && y && w && denom && row_loss, "smer_wce_fwd_bwd: null pointer");
  if (R == 0) return SMER_OK;
  hipStream_t s = (hipStream_t)stream;
  dim3 grid((R + 3) / 4);
  if (dtype == SMER_BF16)
    hipLaunchKernelGGL(wce_kernel<bf16>, grid, dim3(256), 0, s, R, V, logits, ldl, y, w, denom,
                       row_loss, (bf16*)dlogits, ldd, grad_scale);
  else if (dtype == SMER_F32)
    hipLaunchKernelGGL(wce_kernel<float>, grid, dim3(256), 0, s, R, V, logits, ldl, y, w, denom,
                       row_loss, (float*)dlogits, ldd, grad_scale);
  else
    return smer_set_error(SMER_ERR_UNSUPPORTED, "smer_wce_fwd_bwd: dtype");
  if (loss_out)
    hipLaunchKernelGGL(sum_div_kernel, dim3(1), dim3(256), 0, s, R, row_loss, denom, loss_out);
  SMER_CHECK_LAUNCH("smer_wce_fwd_bwd");
  return SMER_OK;
}

template <typename T>
static void wce_ex_launch(bool ls_on, dim3 grid, hipStream_t s, int R, int V, const float* logits, long ldl,
                          const int64_t* y, const float* w, const float* denom, float* row_loss,
                          float* row_nll, void* dlogits, long ldd, float grad_scale, float ls) {
  if (ls_on)
    hipLaunchKernelGGL((wce_ex_kernel<T, true>), grid, dim3(256), 0, s, R, V, logits, ldl, y, w, denom,
                       row_loss, row_nll, (T*)dlogits, ldd, grad_scale, ls);
  else
    hipLaunchKernelGGL((wce_ex_kernel<T, false>), grid, dim3(256), 0, s, R, V, logits, ldl, y, w, denom,
                       row_loss, row_nll, (T*)dlogits, ldd, grad_scale, ls);
}

extern "C" int smer_wce_fwd_bwd_ex(int dtype, int R, int V, const float* logits, long ldl,
                                   const int64_t* y, const float* w, const float* denom,
                                   float* row_loss, float* loss_out, void* dlogits, long ldd,
                                   float grad_scale, float label_smoothing, float* row_nll,
                                   smer_stream_t stream) {
  SMER_REQUIRE(logits && y && w && denom && row_loss, "smer_wce_fwd_bwd_ex: null pointer");
  SMER_REQUIRE(label_smoothing >= 0.f && label_smoothing < 1.f,  // also NaN
               "smer_wce_fwd_bwd_ex: label_smoothing must be in [0, 1)");
  if (R == 0) return SMER_OK;
  hipStream_t s = (hipStream_t)stream;
  dim3 grid((R + 3) / 4);
  const bool ls_on = label_smoothing > 0.f;
  if (dtype == SMER_BF16)
    wce_ex_launch<bf16>(ls_on, grid, s, R, V, logits, ldl, y, w, denom, row_loss, row_nll, dlogits, ldd,
                        grad_scale, label_smoothing);
  else if (dtype == SMER_F32)
    wce_ex_launch<float>(ls_on, grid, s, R, V, logits, ldl, y, w, denom, row_loss, row_nll, dlogits, ldd,
                         grad_scale, label_smoothing);
  else
    return smer_set_error(SMER_ERR_UNSUPPORTED, "smer_wce_fwd_bwd_ex: dtype");
  if (loss_out)
    hipLaunchKernelGGL(sum_div_kernel, dim3(1), dim3(256), 0, s, R, row_loss, denom, loss_out);
  SMER_CHECK_LAUNCH("smer_wce_fwd_bwd_ex");
  return SMER_OK;
}

extern "C" int smer_adam(long n, float* p, const float* g, float* m, float* v, void* p_bf16,
                         float lr, float b1, float b2, float eps, float bc1, float bc2_sqrt,
                         smer_stream_t stream) {
  SMER_REQUIRE(p && g && m && v, "smer_adam: null pointer");
  if (n == 0) return SMER_OK;
  long blocks = (n + 255) / 256;
  if (blocks > 8192) blocks = 8192;
  hipLaunchKernelGGL(adam_kernel<false>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, n, p, g, m, v,
                     (bf16*)p_bf16, lr, b1, b2, eps, bc1, bc2_sqrt);
  SMER_CHECK_LAUNCH("smer_adam");
  return SMER_OK;
}

extern "C" int smer_adam_guarded(long n, float* p, const float* g, float* m, float* v, void* p_bf16,
                                 float lr, float b1, float b2, float eps, float bc1, float bc2_sqrt,
                                 const float* ctl, smer_stream_t stream) {
  SMER_REQUIRE(p && g && m && v && ctl, "smer_adam_guarded: null pointer");
  SMER_REQUIRE(n >= 0, "smer_adam_guarded: n < 0");
  if (n == 0) return SMER_OK;
  long blocks = (n + 255) / 256;
  if (blocks > 8192) blocks = 8192;
  hipLaunchKernelGGL((adam_kernel<true, const float*>), dim3(blocks), dim3(256), 0, (hipStream_t)stream, n, p, g,
                     m, v, (bf16*)p_bf16, lr, b1, b2, eps, bc1, bc2_sqrt, ctl);
  SMER_CHECK_LAUNCH("smer_adam_guarded");
  return SMER_OK;
}

namespace {
struct AdamExLaunch {
  long n, head, nvec;
  float *p, *m, *v, *ema;
  const float *g, *ctl;
  bf16* pb;
  AdamExArgs a;
  hipStream_t stream;
};

template <bool GUARDED, int WD, bool EMA>
void adam_ex_launch(const AdamExLaunch& l) {
  const long nscalar = l.n - 4 * l.nvec;
  long blocks = ((l.nvec > nscalar ? l.nvec : nscalar) + 255) / 256;
  if (blocks > 8192) blocks = 8192;
  hipLaunchKernelGGL((adam_ex_kernel<GUARDED, WD, EMA>), dim3(blocks), dim3(256), 0, l.stream, l.n, l.head,
                     l.nvec, l.p, l.g, l.m, l.v, l.pb, l.ema, l.ctl, l.a);
}

template <bool GUARDED, int WD>
void adam_ex_pick_ema(const AdamExLaunch& l) {
  l.ema ? adam_ex_launch<GUARDED, WD, true>(l) : adam_ex_launch<GUARDED, WD, false>(l);
}

template <bool GUARDED>
void adam_ex_pick_wd(const AdamExLaunch& l, int wd_mode) {
  if (wd_mode == 0) adam_ex_pick_ema<GUARDED, 0>(l);
  else if (wd_mode == 1) adam_ex_pick_ema<GUARDED, 1>(l);
  else adam_ex_pick_ema<GUARDED, 2>(l);
}
}  // namespace

extern "C" int smer_adam_ex(long n, float* p, const float* g, float* m, float* v, void* p_bf16, float lr,
                            float b1, float b2, float eps, float bc1, float bc2_sqrt, const float* ctl,
                            float wd, float decay_mul, int decoupled, float* ema, float ema_decay,
                            smer_stream_t stream) {
  SMER_REQUIRE(p && g && m && v, "smer_adam_ex: null pointer");
  SMER_REQUIRE(n >= 0, "smer_adam_ex: n < 0");
  SMER_REQUIRE(__builtin_isfinite(wd) && __builtin_isfinite(decay_mul) && __builtin_isfinite(ema_decay),
               "smer_adam_ex: wd, decay_mul and ema_decay must be finite");
  const uintptr_t a4[5] = {(uintptr_t)p, (uintptr_t)g, (uintptr_t)m, (uintptr_t)v, (uintptr_t)ema};
  SMER_REQUIRE(((a4[0] | a4[1] | a4[2] | a4[3] | a4[4]) & 3) == 0 && ((uintptr_t)p_bf16 & 1) == 0,
               "smer_adam_ex: p, g, m, v, ema must be 4-B aligned, p_bf16 2-B aligned");
  if (n == 0) return SMER_OK;
  // the scalar head ends where p reaches a 16-B boundary; the vector body
  // needs g, m, v, ema on one there too, and the bf16 copy on an 8-B one
  long head = (long)(((16 - (a4[0] & 15)) & 15) / 4);
  if (head > n) head = n;
  bool vec = true;
  for (int k = 1; k < 5; ++k) vec = vec && (a4[k] == 0 || (a4[k] & 15) == (a4[0] & 15));
  if (p_bf16) vec = vec && (((uintptr_t)p_bf16 + 2 * (uintptr_t)head) & 7) == 0;
  if (!vec) head = n;
  AdamExLaunch l;
  l.n = n, l.head = head, l.nvec = (n - head) / 4;
  l.p = p, l.g = g, l.m = m, l.v = v, l.ema = ema, l.ctl = ctl, l.pb = (bf16*)p_bf16;
  l.a = AdamExArgs{lr, b1, b2, eps, bc1, bc2_sqrt, wd, decay_mul, ema_decay};
  l.stream = (hipStream_t)stream;
  const int wd_mode = decoupled ? 2 : (wd != 0.f ? 1 : 0);
  if (ctl) adam_ex_pick_wd<true>(l, wd_mode);
  else adam_ex_pick_wd<false>(l, wd_mode);
  SMER_CHECK_LAUNCH("smer_adam_ex");
  return SMER_OK;
}

extern "C" int smer_adam_groups(long n, float* p, const float* g, float* m, float* v, void* p_bf16,
                                const float* ctl, const uint8_t* gmap, long block0,
                                const smer_adam_group* groups, int ngroups, float* ema, float ema_decay,
                                smer_stream_t stream) {
  SMER_REQUIRE(p && g && m && v && gmap && groups, "smer_adam_groups: null pointer");
  SMER_REQUIRE(n >= 0 && block0 >= 0, "smer_adam_groups: n < 0 or block0 < 0");
  SMER_REQUIRE(n % 64 == 0, "smer_adam_groups: n must be a multiple of 64 (whole parameter slots)");
  SMER_REQUIRE(ngroups >= 1 && ngroups <= SMER_ADAM_MAX_GROUPS,
               "smer_adam_groups: ngroups must be 1..SMER_ADAM_MAX_GROUPS");
  const uintptr_t a16 = (uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v | (uintptr_t)ema;
  SMER_REQUIRE((a16 & 15) == 0 && ((uintptr_t)p_bf16 & 7) == 0,
               "smer_adam_groups: p, g, m, v, ema must be 16-B aligned, p_bf16 8-B aligned");
  SMER_REQUIRE(__builtin_isfinite(ema_decay), "smer_adam_groups: wd, decay_mul and ema_decay must be finite");
  AdamGroupTable tab = {};
  for (int k = 0; k < ngroups; ++k) {
    SMER_REQUIRE(__builtin_isfinite(groups[k].wd) && __builtin_isfinite(groups[k].decay_mul),
                 "smer_adam_groups: wd, decay_mul and ema_decay must be finite");
    SMER_REQUIRE(groups[k].wd_mode >= 0 && groups[k].wd_mode <= 2, "smer_adam_groups: wd_mode must be 0, 1 or 2");
    tab.row[k] = groups[k];
  }
  if (n == 0) return SMER_OK;
  const long nvec = n / 4;
  long blocks = (nvec + 255) / 256;  // adam_ex_launch's rule
  if (blocks > 8192) blocks = 8192;
  bf16* pb = (bf16*)p_bf16;
  const dim3 grid((unsigned)blocks), wg(256);
  hipStream_t s = (hipStream_t)stream;
#define SMER_ADAM_GROUPS_LAUNCH(GUARDED, EMA)                                                                 \
  hipLaunchKernelGGL((adam_groups_kernel<GUARDED, EMA>), grid, wg, 0, s, nvec, p, g, m, v, pb, ema, ctl, gmap, \
                     block0, ema_decay, tab)
  if (ctl) {
    if (ema) SMER_ADAM_GROUPS_LAUNCH(true, true);
    else SMER_ADAM_GROUPS_LAUNCH(true, false);
  } else {
    if (ema) SMER_ADAM_GROUPS_LAUNCH(false, true);
    else SMER_ADAM_GROUPS_LAUNCH(false, false);
  }
#undef SMER_ADAM_GROUPS_LAUNCH
  SMER_CHECK_LAUNCH("smer_adam_groups");
  return SMER_OK;
}

extern "C" long smer_grad_sqnorm_nparts(long n) { return n <= 0 ? 0 : (n + GN_CH - 1) / GN_CH; }

extern "C" int smer_grad_sqnorm_part(long n, const float* g, float* part, smer_stream_t stream) {
  SMER_REQUIRE(n >= 0, "smer_grad_sqnorm_part: n < 0");
  SMER_REQUIRE(g && part, "smer_grad_sqnorm_part: null pointer");
  if (((uintptr_t)g & 15) != 0)
    return smer_set_error(SMER_ERR_UNSUPPORTED, "smer_grad_sqnorm_part: g must be 16-B aligned");
  if (n == 0) return SMER_OK;
  const long nparts = smer_grad_sqnorm_nparts(n);
  SMER_REQUIRE(nparts <= (1L << 23), "smer_grad_sqnorm_part: range too long (2^37 floats at most)");
  hipLaunchKernelGGL(grad_sqnorm_kernel, dim3((unsigned)nparts), dim3(256), 0, (hipStream_t)stream, n, g,
                     part);
  SMER_CHECK_LAUNCH("smer_grad_sqnorm_part");
  return SMER_OK;
}

extern "C" int smer_clip_scale(int nparts, const float* part, float max_norm, float* ctl,
                               smer_stream_t stream) {
  SMER_REQUIRE(nparts >= 0, "smer_clip_scale: nparts < 0");
  SMER_REQUIRE(ctl && (part || nparts == 0), "smer_clip_scale: null pointer");
  SMER_REQUIRE(max_norm > 0.f, "smer_clip_scale: max_norm must be > 0 (inf allowed, NaN not)");
  hipLaunchKernelGGL(clip_scale_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, nparts, part,
                     max_norm, ctl);
  SMER_CHECK_LAUNCH("smer_clip_scale");
  return SMER_OK;
}

extern "C" int smer_cast(int src_dtype, int dst_dtype, long n, const void* src, void* dst,
                         smer_stream_t stream) {
  if (n == 0) return SMER_OK;
  long blocks = (n + 255) / 256;
  if (blocks > 8192) blocks = 8192;
  hipStream_t s = (hipStream_t)stream;
  if (src_dtype == SMER_F32 && dst_dtype == SMER_BF16)
    hipLaunchKernelGGL((cast_kernel<float, bf16>), dim3(blocks), dim3(256), 0, s, n,
                       (const float*)src, (bf16*)dst);
  else if (src_dtype == SMER_BF16 && dst_dtype == SMER_F32)
    hipLaunchKernelGGL((cast_kernel<bf16, float>), dim3(blocks), dim3(256), 0, s, n,
                       (const bf16*)src, (float*)dst);
  else if (src_dtype == SMER_F32 && dst_dtype == SMER_F32)
    hipLaunchKernelGGL((cast_kernel<float, float>), dim3(blocks), dim3(256), 0, s, n,
                       (const float*)src, (float*)dst);
  else if (src_dtype == SMER_BF16 && dst_dtype == SMER_BF16)
    hipLaunchKernelGGL((cast_kernel<bf16, bf16>), dim3(blocks), dim3(256), 0, s, n,
                       (const bf16*)src, (bf16*)dst);
  else
    return smer_set_error(SMER_ERR_UNSUPPORTED, "smer_cast: dtype");
  SMER_CHECK_LAUNCH("smer_cast");
  return SMER_OK;
}

template <typename S, typename D>
__global__ void cast2d_kernel(int rows, int cols, const S* __restrict__ s, long lds,
                              D* __restrict__ d, long ldd) {
  long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long)rows * cols) return;
  int r = idx / cols, c = idx % cols;
  d[(long)r * ldd + c] = from_f32<D>(to_f32(s[(long)r * lds + c]));
}

extern "C" int smer_cast2d(int src_dtype, int dst_dtype, int rows, int cols, const void* src,
                           long lds, void* dst, long ldd, smer_stream_t stream) {
  long n = (long)rows * cols;
  if (n == 0) return SMER_OK;
  hipStream_t s = (hipStream_t)stream;
  dim3 g((n + 255) / 256);
  if (src_dtype == SMER_F32 && dst_dtype == SMER_BF16)
    hipLaunchKernelGGL((cast2d_kernel<float, bf16>), g, dim3(256), 0, s, rows, cols, (const float*)src, lds, (bf16*)dst, ldd);
  else if (src_dtype == SMER_F32 && dst_dtype == SMER_F32)
    hipLaunchKernelGGL((cast2d_kernel<float, float>), g, dim3(256), 0, s, rows, cols, (const float*)src, lds, (float*)dst, ldd);
  else if (src_dtype == SMER_BF16 && dst_dtype == SMER_F32)
    hipLaunchKernelGGL((cast2d_kernel<bf16, float>), g, dim3(256), 0, s, rows, cols, (const bf16*)src, lds, (float*)dst, ldd);
  else if (src_dtype == SMER_BF16 && dst_dtype == SMER_BF16)
    hipLaunchKernelGGL((cast2d_kernel<bf16, bf16>), g, dim3(256), 0, s, rows, cols, (const bf16*)src, lds, (bf16*)dst, ldd);
  else
    return smer_set_error(SMER_ERR_UNSUPPORTED, "smer_cast2d: dtype");
  SMER_CHECK_LAUNCH("smer_cast2d");
  return SMER_OK;
}

extern "C" size_t smer_colsum_workspace(int M, int N) {
  size_t nblk = (size_t)(M + CS_ROWS - 1) / CS_ROWS;
  return nblk * N * sizeof(float) + smer_col_reduce_scratch((int)nblk, N);
}

extern "C" int smer_colsum(int dtype, int M, int N, const void* x, long ldx, float* out,
                           int accumulate, void* workspace, size_t ws_bytes,
                           smer_stream_t stream) {
  SMER_REQUIRE(x && out, "smer_colsum: null pointer");
  SMER_REQUIRE(workspace && ws_bytes >= smer_colsum_workspace(M, N), "smer_colsum: workspace");
  if (N == 0) return SMER_OK;
  hipStream_t s = (hipStream_t)stream;
  int nblk = (M + CS_ROWS - 1) / CS_ROWS;
  dim3 grid((N + 511) / 512, nblk > 0 ? nblk : 1);
  bool vec = ((uintptr_t)x & 15) == 0 && ldx % 8 == 0;
  if (M > 0) {
    if (dtype == SMER_BF16) {
      if (vec) hipLaunchKernelGGL((colsum_part_kernel<bf16, true>), grid, dim3(256), 0, s, M, N, (const bf16*)x, ldx, (float*)workspace);
      else hipLaunchKernelGGL((colsum_part_kernel<bf16, false>), grid, dim3(256), 0, s, M, N, (const bf16*)x, ldx, (float*)workspace);
    } else if (dtype == SMER_F32) {
      if (vec) hipLaunchKernelGGL((colsum_part_kernel<float, true>), grid, dim3(256), 0, s, M, N, (const float*)x, ldx, (float*)workspace);
      else hipLaunchKernelGGL((colsum_part_kernel<float, false>), grid, dim3(256), 0, s, M, N, (const float*)x, ldx, (float*)workspace);
    } else {
      return smer_set_error(SMER_ERR_UNSUPPORTED, "smer_colsum: dtype");
    }
  }
  smer_col_reduce_launch(nblk, N, (const float*)workspace, (long)N, 0L, out, accumulate, 1.f,
                         (float*)workspace + (size_t)nblk * N, s);
  SMER_CHECK_LAUNCH("smer_colsum");
  return SMER_OK;
}

// ---------------------------------------------------------------------------
// Debug checksum (repeatability probes, tools/ck_log.py): partial[b] =
// sum over the 4-byte words w_i of a strided 2-D region of w_i * (2 i + 1)
// (mod 2^64), word i = r * (row_bytes / 4) + c, block b taking every
// nparts-th row.  The host adds the partials; the sum is order-independent,
// so two runs over the same bits give the same value.  One launch on the
// caller's stream, no allocation, no sync.
__global__ __launch_bounds__(256) void checksum_kernel(const uint32_t* __restrict__ p, long rows,
                                                       long row_words, long ld_words,
                                                       unsigned long long* __restrict__ out) {
  __shared__ unsigned long long red[256];
  unsigned long long a = 0;
  for (long r = blockIdx.x; r < rows; r += gridDim.x) {
    const uint32_t* row = p + r * ld_words;
    const unsigned long long base = (unsigned long long)r * (unsigned long long)row_words;
    for (long c = threadIdx.x; c < row_words; c += 256)
      a += (unsigned long long)row[c] * (2ull * (base + (unsigned long long)c) + 1ull);
  }
  red[threadIdx.x] = a;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[blockIdx.x] = red[0];
}

extern "C" int smer_debug_checksum(const void* p, long rows, long row_bytes, long ld_bytes,
                                   unsigned long long* out, int nparts, smer_stream_t stream) {
  SMER_REQUIRE(p && out, "smer_debug_checksum: null pointer");
  SMER_REQUIRE(row_bytes % 4 == 0 && ld_bytes % 4 == 0 && ((uintptr_t)p & 3) == 0 && nparts > 0,
               "smer_debug_checksum: 4-byte words only");
  hipLaunchKernelGGL(checksum_kernel, dim3(nparts), dim3(256), 0, (hipStream_t)stream,
                     (const uint32_t*)p, rows, row_bytes / 4, ld_bytes / 4, out);
  SMER_CHECK_LAUNCH("smer_debug_checksum");
  return SMER_OK;
}

// ---------------------------------------------------------------------------
// Validation accuracy (train.py:988-1034 `accuracy`, as validate() calls it):
// one wave per row; pred = the first index of the row's max logit
// (torch.argmax), target y; rows whose target is the pad index are skipped;
// counts[2 c] += 1 and counts[2 c + 1] += (pred == y) for the target's token
// class c = cls[y], and the same for the total in the last pair (c = ncls).
// Integer atomics: the counts are exact and order-independent.
__global__ __launch_bounds__(256) void argmax_acc_kernel(int R, int V, const float* __restrict__ logits,
                                                         long ldl, const int64_t* __restrict__ y,
                                                         const int32_t* __restrict__ cls, int ncls,
                                                         int pad, unsigned* __restrict__ counts) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= R) return;
  const long yt = y[r];
  if (yt == pad) return;
  const float* x = logits + (long)r * ldl;
  float best = -INFINITY;
  int bi = V;  // V: no finite value seen yet (all -inf: index 0, as torch)
  // a NaN beats any number and the first NaN wins, as torch.argmax orders them
  for (int v = lane; v < V; v += 64) {
    const float xv = x[v];
    // per lane: ascending v, first max (or first NaN) kept
    if (bi == V || (xv != xv ? best == best : xv > best)) { best = xv; bi = v; }
  }
#pragma unroll
  for (int w = 1; w < 64; w <<= 1) {
    const float ob = __shfl_xor(best, w, 64);
    const int oi = __shfl_xor(bi, w, 64);
    const bool on = ob != ob, bn = best != best;
    if (on ? (!bn || oi < bi) : (!bn && (ob > best || (ob == best && oi < bi)))) { best = ob; bi = oi; }
  }
  if (lane == 0) {
    const int c = (yt >= 0 && yt < V) ? cls[yt] : ncls;
    const unsigned hit = (long)bi == yt ? 1u : 0u;
    if (c >= 0 && c < ncls) {
      atomicAdd(counts + 2 * c, 1u);
      atomicAdd(counts + 2 * c + 1, hit);
    }
    atomicAdd(counts + 2 * ncls, 1u);
    atomicAdd(counts + 2 * ncls + 1, hit);
  }
}

extern "C" int smer_argmax_accuracy(int R, int V, const float* logits, long ldl, const int64_t* y,
                                    const int32_t* cls, int ncls, int pad, unsigned* counts,
                                    smer_stream_t stream) {
  SMER_REQUIRE(R >= 0 && V > 0 && ncls >= 0, "smer_argmax_accuracy: bad sizes");
  SMER_REQUIRE(logits && y && cls && counts, "smer_argmax_accuracy: null pointer");
  if (R == 0) return SMER_OK;
  hipLaunchKernelGGL(argmax_acc_kernel, dim3((R + 3) / 4), dim3(256), 0, (hipStream_t)stream, R, V, logits,
                     ldl, y, cls, ncls, pad, counts);
  SMER_CHECK_LAUNCH("smer_argmax_accuracy");
  return SMER_OK;
}
