// ComplEx decoder on scored triples (Trouillon et al. 2016; an extension): the sampled-negative objective scores triples
// one by one, so the trilinear product over complex numbers needs kernels of its own -- the all-candidate routes of rgcn_rank.hip serve
// ComplEx through their query pass alone.  Contract: include/rgcn_hip.h (rgcn_complex_*).
//
// A row of the entity or the relation table, d = 2 h wide, holds h complex features: real parts in columns [0, h), imaginary parts in
// [h, d).  With s, r, o the rows of a triple and g the gradient of its score
//     score   = Re sum_k s[k] r[k] conj(o[k])
//     d/d s   = g conj(r) o        d/d o = g s r        d/d r = g conj(s) o           (each read as [Re | Im])
// Every kernel gives a lane FOUR ADJACENT complex features per pass of 256: two 16-byte pieces of an fp32 row (at f and at h + f), two
// 8-byte pieces of a bf16 row, when h % 4 == 0 and the tables are aligned (VEC; the launchers decide, as the DistMult ones do), element
// by element otherwise.  Sums are fp32.  The roles and their signatures are DistMult's (rgcn_kernels.hip): the scoring kernel carries the
// counting pass of the backward's two CSRs, the entity gradients come from one wave per entity over those CSRs without atomics, the
// relation and bias gradients from predicate-sorted triples with one atomic per run and feature.  There is no twin of DistMult's
// LDS-table route nor of its atomic scatter.
#include <cstdlib>

#include "rgcn_device.h"      // HIP_TRY, f32x4, WG, zero_async, aligned, the bf16 widen / round helpers

namespace {

struct C4 { f32x4 re, im; };     // four adjacent complex features

// complex features f .. f + 3 of row `row` of a table of h complex features per row.  BF: bf16 rows.  VEC: f + 3 < h and the pieces
// are aligned (a lane past the row's end passes f = 0 and keeps nothing); else features past h read as 0.
template <bool BF, bool VEC>
__device__ __forceinline__ C4 load_c4(const void *__restrict__ table, long long row, int h, int f) {
  C4 v;
  if constexpr (BF) {
    const uint16_t *p = static_cast<const uint16_t *>(table) + (size_t)row * (2 * h);
    if (VEC) {
      const float4 a = bf16x4_widen(*reinterpret_cast<const uint2 *>(p + f)), b = bf16x4_widen(*reinterpret_cast<const uint2 *>(p + h + f));
      v.re = f32x4{a.x, a.y, a.z, a.w};
      v.im = f32x4{b.x, b.y, b.z, b.w};
    } else {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const bool in = f + q < h;
        v.re[q] = in ? bf16_widen(p[f + q]) : 0.f;
        v.im[q] = in ? bf16_widen(p[h + f + q]) : 0.f;
      }
    }
  } else {
    const float *p = static_cast<const float *>(table) + (size_t)row * (2 * h);
    if (VEC) {
      v.re = *reinterpret_cast<const f32x4 *>(p + f);
      v.im = *reinterpret_cast<const f32x4 *>(p + h + f);
    } else {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const bool in = f + q < h;
        v.re[q] = in ? p[f + q] : 0.f;
        v.im[q] = in ? p[h + f + q] : 0.f;
      }
    }
  }
  return v;
}

__device__ __forceinline__ C4 cmul(const C4 &a, const C4 &b) { return {a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re}; }     // a b
__device__ __forceinline__ C4 cmulc(const C4 &a, const C4 &b) { return {a.re * b.re + a.im * b.im, a.re * b.im - a.im * b.re}; }    // conj(a) b

// one wave per triple; the CSR counting pass rides along exactly as in distmult_fwd_kernel
template <bool BF, bool VEC>
__global__ __launch_bounds__(WG) void complex_fwd_kernel(
    const long long *__restrict__ tr, long long T, const void *__restrict__ nodes, const float *__restrict__ rel,
    const float *__restrict__ sb, const float *__restrict__ pb, const float *__restrict__ ob,
    float *__restrict__ scores, int h, long long n_nodes, int n_rel, int *__restrict__ err, int *__restrict__ counts,
    int *__restrict__ ranks) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const long long wstride = (long long)gridDim.x * (WG / 64);
  for (long long t = (long long)blockIdx.x * (WG / 64) + wave; t < T; t += wstride) {
    const long long s = tr[3 * t], p = tr[3 * t + 1], o = tr[3 * t + 2];
    if (s < 0 || s >= n_nodes || o < 0 || o >= n_nodes || p < 0 || p >= n_rel) {   // the reference raises IndexError here
      if (lane == 0) { if (err) atomicMax(err, 1); scores[t] = 0.f; }
      continue;
    }
    int rk_s = 0, rk_o = 0;
    if (counts && lane == 0) { rk_s = atomicAdd(counts + 1 + s, 1); rk_o = atomicAdd(counts + n_nodes + 2 + o, 1); }
    float a = 0.f;
    for (int f = 4 * lane; f < h; f += 256) {
      const C4 x = load_c4<BF, VEC>(nodes, s, h, f), w = load_c4<false, VEC>(rel, p, h, f), y = load_c4<BF, VEC>(nodes, o, h, f);
      const C4 z = cmul(x, w);
      const f32x4 q = z.re * y.re + z.im * y.im;                // Re(z conj(y))
      a += (q[0] + q[1]) + (q[2] + q[3]);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) a += __shfl_xor(a, off, 64);
    if (lane == 0) {
      if (sb) a += sb[s] + pb[p] + ob[o];
      scores[t] = a;
      if (counts) *reinterpret_cast<int2 *>(ranks + 2 * t) = make_int2(rk_s, rk_o);
    }
  }
}

// Entity gradients: one wave per entity over the two CSRs of the scored triples (rgcn_distmult_csr_place: int4 entries {other end,
// predicate, score gradient (bits), -}), the walk of distmult_bwd_all_kernel<3, VEC, false, BF> -- the lanes load 64 entries in one round
// trip and hand them to the wave four at a time with v_readlane, four entity rows and four relation rows in flight per step.
//     dnodes[n] = sum_{t: s_t = n} g_t conj(r[p_t]) nodes[o_t]  +  sum_{t: o_t = n} g_t nodes[s_t] r[p_t]
// Both sides meet in the registers of the wave; the row is written once (bf16: the fp32 sum rounded once).
template <bool BF, bool VEC>
__global__ __launch_bounds__(WG) void complex_bwd_nodes_kernel(
    const int *__restrict__ rp_s, const int *__restrict__ rp_o, const int4 *__restrict__ entries, const void *__restrict__ nodes,
    const float *__restrict__ rel, void *__restrict__ dnodes, long long N, int h) {
  const int lane = threadIdx.x & 63;
  const long long wave0 = ((long long)blockIdx.x * WG + threadIdx.x) >> 6, nw = ((long long)gridDim.x * WG) >> 6;
  for (long long n = wave0; n < N; n += nw) {
    for (int f0 = 0; f0 < h; f0 += 256) {
      const int f = f0 + 4 * lane;
      const bool act = f < h;
      const int fl = VEC && !act ? 0 : f;                 // VEC: lanes past the row's end load from feature 0 and keep nothing
      C4 acc = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
      for (int side = 0; side < 2; ++side) {
        const int *rp = side ? rp_o : rp_s;
        const int e0 = __builtin_amdgcn_readfirstlane(rp[n]), e1 = __builtin_amdgcn_readfirstlane(rp[n + 1]);
        for (int c0 = e0; c0 < e1; c0 += 64) {
          const int cnt = min(64, e1 - c0);
          const int4 me = entries[c0 + min(lane, cnt - 1)];      // lanes past the row's end repeat its last entry, with a zero gradient
          const int mo = me.x, mr = me.y, mg = lane < cnt ? me.z : 0;
          for (int j = 0; j < cnt; j += 4) {
            C4 xe[4], we[4];
            float ge[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
              const int oe = __builtin_amdgcn_readlane(mo, j + u), pe = __builtin_amdgcn_readlane(mr, j + u);
              ge[u] = __int_as_float(__builtin_amdgcn_readlane(mg, j + u));
              xe[u] = load_c4<BF, VEC>(nodes, oe, h, fl);
              we[u] = load_c4<false, VEC>(rel, pe, h, fl);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
              const C4 c = side ? cmul(xe[u], we[u]) : cmulc(we[u], xe[u]);      // object rows: s r; subject rows: conj(r) o
              acc.re += c.re * ge[u];
              acc.im += c.im * ge[u];
            }
          }
        }
      }
      if constexpr (BF) {
        uint16_t *oh = static_cast<uint16_t *>(dnodes) + (size_t)n * (2 * h);
        if (VEC) {
          if (act) {
            *reinterpret_cast<uint2 *>(oh + f) = bf16x4_round(make_float4(acc.re[0], acc.re[1], acc.re[2], acc.re[3]));
            *reinterpret_cast<uint2 *>(oh + h + f) = bf16x4_round(make_float4(acc.im[0], acc.im[1], acc.im[2], acc.im[3]));
          }
        } else {
#pragma unroll
          for (int q = 0; q < 4; ++q)
            if (f + q < h) { oh[f + q] = bf16_round(acc.re[q]); oh[h + f + q] = bf16_round(acc.im[q]); }
        }
      } else {
        float *o = static_cast<float *>(dnodes) + (size_t)n * (2 * h);
        if (VEC) {
          if (act) { *reinterpret_cast<f32x4 *>(o + f) = acc.re; *reinterpret_cast<f32x4 *>(o + h + f) = acc.im; }
        } else {
#pragma unroll
          for (int q = 0; q < 4; ++q)
            if (f + q < h) { o[f + q] = acc.re[q]; o[h + f + q] = acc.im[q]; }
        }
      }
    }
  }
}

// Relation and bias gradients: each wave walks 64 consecutive triples of the predicate-sorted list (distmult_bwd_kernel with skip_nodes),
// a relation's run is summed in registers and flushed with one fp32 atomic per run and feature: drel[p] += g conj(s) o.
template <bool BF, bool VEC>
__global__ __launch_bounds__(WG) void complex_bwd_rel_kernel(
    const long long *__restrict__ tr, long long T, const void *__restrict__ nodes, const float *__restrict__ gs, float *__restrict__ drel,
    float *__restrict__ dsb, float *__restrict__ dpb, float *__restrict__ dob, int h, long long n_nodes, int n_rel) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const long long wstride = (long long)gridDim.x * (WG / 64) * 64;
  for (long long t0 = ((long long)blockIdx.x * (WG / 64) + wave) * 64; t0 < T; t0 += wstride) {
    const long long t1 = min(T, t0 + 64);
    for (int f0 = 0; f0 < h; f0 += 256) {
      const int f = f0 + 4 * lane;
      const bool act = f < h;
      const int fl = VEC && !act ? 0 : f;
      C4 acc = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
      long long cur = -1;
      auto flush = [&]() {
        float *row = drel + (size_t)cur * (2 * h);
#pragma unroll
        for (int q = 0; q < 4; ++q)
          if (f + q < h) { atomicAdd(row + f + q, acc.re[q]); atomicAdd(row + h + f + q, acc.im[q]); }
      };
      for (long long t = t0; t < t1; ++t) {
        const long long s = tr[3 * t], p = tr[3 * t + 1], o = tr[3 * t + 2];
        if (s < 0 || s >= n_nodes || o < 0 || o >= n_nodes || p < 0 || p >= n_rel) continue;   // flagged by the forward
        if (p != cur) {
          if (cur >= 0) flush();
          acc = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
          cur = p;
        }
        const float g = gs[t];
        const C4 c = cmulc(load_c4<BF, VEC>(nodes, s, h, fl), load_c4<BF, VEC>(nodes, o, h, fl));
        acc.re += c.re * g;
        acc.im += c.im * g;
        if (f0 == 0 && dsb && lane == 0) {
          atomicAdd(&dsb[s], g);
          atomicAdd(&dpb[p], g);
          atomicAdd(&dob[o], g);
        }
      }
      if (cur >= 0) flush();
    }
  }
}

// the argument rule every entry shares: real halves | imaginary halves
inline bool odd_width(const char *name, int32_t d) {
  if (d > 0 && (d & 1)) {
    rgcn_set_error("%s: ComplEx rows hold real halves | imaginary halves and need an even width, got d = %d", name, (int)d);
    return true;
  }
  return false;
}

template <bool BF>
int complex_fwd(const char *name, const int64_t *triples, int64_t T, const void *nodes, const float *rel, const float *sbias, const float *pbias,
                const float *obias, float *scores, int64_t n_nodes, int32_t n_rel, int32_t d, int32_t *err_flag, int32_t *rank_counts,
                int32_t *ranks, void *stream) {
  if (T < 0 || d <= 0 || (T && (!triples || !nodes || !rel || !scores)) || (rank_counts != nullptr) != (ranks != nullptr) ||
      (rank_counts && (n_nodes <= 0 || 2 * T > INT32_MAX))) { rgcn_set_error("%s: bad argument", name); return RGCN_EINVAL; }
  if (odd_width(name, d)) return RGCN_EINVAL;
  if ((sbias != nullptr) != (pbias != nullptr) || (sbias != nullptr) != (obias != nullptr)) { rgcn_set_error("%s: biases must be all set or all NULL", name); return RGCN_EINVAL; }
  hipStream_t st = (hipStream_t)stream;
  if (err_flag) HIP_TRY(zero_async(err_flag, sizeof(int32_t), st));
  if (rank_counts) HIP_TRY(zero_async(rank_counts, (size_t)(2 * n_nodes + 3) * sizeof(int32_t), st));
  if (T == 0) return RGCN_OK;
  const unsigned gx = (unsigned)std::min<int64_t>((T + 3) / 4, 256 * 32);
  const int h = d / 2;
  auto go = [&](auto k) {
    hipLaunchKernelGGL(k, dim3(gx), dim3(WG), 0, st, reinterpret_cast<const long long *>(triples), (long long)T, nodes, rel, sbias, pbias, obias,
                       scores, h, (long long)n_nodes, n_rel, err_flag, rank_counts, ranks);
  };
  // pieces of four complex features: 16 bytes of an fp32 row, 8 of a bf16 row, 16 of the relation table
  if (h % 4 == 0 && aligned(nodes, BF ? 8 : 16) && aligned(rel, 16)) go(complex_fwd_kernel<BF, true>);
  else go(complex_fwd_kernel<BF, false>);
  HIP_TRY(hipGetLastError());
  return RGCN_OK;
}

template <bool BF>
int complex_bwd_nodes(const char *name, const int32_t *rowptr_s, const int32_t *rowptr_o, const int32_t *entries, const void *nodes,
                      const float *rel, void *dnodes, int64_t n_nodes, int32_t d, void *stream) {
  if (!rowptr_s || !rowptr_o || !nodes || !rel || !dnodes || n_nodes < 0 || d <= 0) { rgcn_set_error("%s: bad argument", name); return RGCN_EINVAL; }
  if (odd_width(name, d)) return RGCN_EINVAL;
  if (!n_nodes) return RGCN_OK;
  const unsigned gx = (unsigned)std::min<int64_t>((n_nodes + 3) / 4, 256 * 32);
  const int h = d / 2;
  auto go = [&](auto k) {
    hipLaunchKernelGGL(k, dim3(gx), dim3(WG), 0, (hipStream_t)stream, rowptr_s, rowptr_o, reinterpret_cast<const int4 *>(entries), nodes, rel,
                       dnodes, (long long)n_nodes, h);
  };
  if (h % 4 == 0 && aligned(nodes, BF ? 8 : 16) && aligned(dnodes, BF ? 8 : 16) && aligned(rel, 16)) go(complex_bwd_nodes_kernel<BF, true>);
  else go(complex_bwd_nodes_kernel<BF, false>);
  HIP_TRY(hipGetLastError());
  return RGCN_OK;
}

template <bool BF>
int complex_bwd_rel(const char *name, const int64_t *triples, int64_t T, const void *nodes, const float *rel, const float *gs, float *drel,
                    float *dsbias, float *dpbias, float *dobias, int64_t n_nodes, int32_t n_rel, int32_t d, void *stream) {
  if (T < 0 || d <= 0 || n_nodes < 0 || n_rel <= 0 || !drel || (T && (!triples || !nodes || !rel || !gs))) { rgcn_set_error("%s: bad argument", name); return RGCN_EINVAL; }
  if (odd_width(name, d)) return RGCN_EINVAL;
  if ((dsbias != nullptr) != (dpbias != nullptr) || (dsbias != nullptr) != (dobias != nullptr)) { rgcn_set_error("%s: bias gradients must be all set or all NULL", name); return RGCN_EINVAL; }
  hipStream_t st = (hipStream_t)stream;
  HIP_TRY(zero_async(drel, (size_t)n_rel * d * sizeof(float), st));
  if (dsbias) {
    HIP_TRY(zero_async(dsbias, (size_t)n_nodes * sizeof(float), st));
    HIP_TRY(zero_async(dobias, (size_t)n_nodes * sizeof(float), st));
    HIP_TRY(zero_async(dpbias, (size_t)n_rel * sizeof(float), st));
  }
  if (T == 0) return RGCN_OK;
  const unsigned gx = (unsigned)std::min<int64_t>((T + 255) / 256, 256 * 32);
  const int h = d / 2;
  auto go = [&](auto k) {
    hipLaunchKernelGGL(k, dim3(gx), dim3(WG), 0, st, reinterpret_cast<const long long *>(triples), (long long)T, nodes, gs, drel, dsbias, dpbias,
                       dobias, h, (long long)n_nodes, n_rel);
  };
  if (h % 4 == 0 && aligned(nodes, BF ? 8 : 16)) go(complex_bwd_rel_kernel<BF, true>);
  else go(complex_bwd_rel_kernel<BF, false>);
  HIP_TRY(hipGetLastError());
  return RGCN_OK;
}

}  // namespace

extern "C" int rgcn_complex_fwd_f32(const int64_t *triples, int64_t T, const float *nodes, const float *rel,
                                    const float *sbias, const float *pbias, const float *obias, float *scores,
                                    int64_t n_nodes, int32_t n_rel, int32_t d, int32_t *err_flag, int32_t *rank_counts,
                                    int32_t *ranks, void *stream) {
  return complex_fwd<false>("complex_fwd", triples, T, nodes, rel, sbias, pbias, obias, scores, n_nodes, n_rel, d, err_flag, rank_counts, ranks, stream);
}

extern "C" int rgcn_complex_fwd_bf16(const int64_t *triples, int64_t T, const uint16_t *nodes, const float *rel,
                                     const float *sbias, const float *pbias, const float *obias, float *scores,
                                     int64_t n_nodes, int32_t n_rel, int32_t d, int32_t *err_flag, int32_t *rank_counts,
                                     int32_t *ranks, void *stream) {
  return complex_fwd<true>("complex_fwd_bf16", triples, T, nodes, rel, sbias, pbias, obias, scores, n_nodes, n_rel, d, err_flag, rank_counts, ranks,
                           stream);
}

extern "C" int rgcn_complex_bwd_nodes_f32(const int32_t *rowptr_s, const int32_t *rowptr_o, const int32_t *entries, const float *nodes,
                                          const float *rel, float *dnodes, int64_t n_nodes, int32_t d, void *stream) {
  return complex_bwd_nodes<false>("complex_bwd_nodes", rowptr_s, rowptr_o, entries, nodes, rel, dnodes, n_nodes, d, stream);
}

extern "C" int rgcn_complex_bwd_nodes_bf16(const int32_t *rowptr_s, const int32_t *rowptr_o, const int32_t *entries, const uint16_t *nodes,
                                           const float *rel, uint16_t *dnodes, int64_t n_nodes, int32_t d, void *stream) {
  return complex_bwd_nodes<true>("complex_bwd_nodes_bf16", rowptr_s, rowptr_o, entries, nodes, rel, dnodes, n_nodes, d, stream);
}

extern "C" int rgcn_complex_bwd_rel_f32(const int64_t *triples, int64_t T, const float *nodes, const float *rel,
                                        const float *gs, float *drel, float *dsbias, float *dpbias, float *dobias,
                                        int64_t n_nodes, int32_t n_rel, int32_t d, void *stream) {
  return complex_bwd_rel<false>("complex_bwd_rel", triples, T, nodes, rel, gs, drel, dsbias, dpbias, dobias, n_nodes, n_rel, d, stream);
}

extern "C" int rgcn_complex_bwd_rel_bf16(const int64_t *triples, int64_t T, const uint16_t *nodes, const float *rel,
                                         const float *gs, float *drel, float *dsbias, float *dpbias, float *dobias,
                                         int64_t n_nodes, int32_t n_rel, int32_t d, void *stream) {
  return complex_bwd_rel<true>("complex_bwd_rel_bf16", triples, T, nodes, rel, gs, drel, dsbias, dpbias, dobias, n_nodes, n_rel, d, stream);
}
