// Ranking evaluator of the link-prediction experiments: every entity scored as the
// head or the tail of each test triple, known true triples masked, rank of the target counted with ties.
// Reference lines taken over: utils/misc.py:60-110 (evaluate: toscore expansion :78-83, model call :85,
// filter_scores :40-58, raw_ranks / num_ties :93-99) and torch_rgcn/layers.py:87-98 (DistMult.forward on the
// expanded [bn, N, 3] index tensor, which is what the reference scores -- three gathers of bn x N x d floats).
//
// Here the [bn, N, 3] index tensor is never built.  For a batch of Q queries
//     scores[q, n] = sum_k (nodes[fixed_q, k] * rel[p_q, k]) * nodes[n, k]  (+ biases)
// is an NT product of the Q x d query vectors with the N x d entity table: fp32 MFMA (v_mfma_f32_16x16x4_f32,
// exact fp32 products and accumulation).  Default kernel: 128 x 128 scores per workgroup, operand slabs staged through
// double-buffered LDS (score_all_lds_kernel); the register-only variant (operands straight from L2, each lane's float4
// feeding four MFMAs of each tile that shares it) is kept selectable for comparison (RGCN_RANK_TILE=44).
// The K index is permuted -- lane group kq carries k = 16t + 4kq + c at MFMA c of step t -- which is legal
// because both operands use the same permutation and the sum over k does not care.
#include <cmath>
#include <cstdlib>

#include "rgcn_device.h"      // HIP_TRY, f32x4, WG, the bf16 widen / round helpers

namespace {

// query vectors and the query-side bias terms; one wave per query
__global__ __launch_bounds__(WG) void rank_query_kernel(
    const long long *__restrict__ batch, int Q, int head, const float *__restrict__ nodes,
    const float *__restrict__ rel, const float *__restrict__ sbias, const float *__restrict__ pbias,
    const float *__restrict__ obias, float *__restrict__ qvec, float *__restrict__ qb, int d) {
  const int q = blockIdx.x * (WG / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (q >= Q) return;
  const long long s = batch[3 * q], p = batch[3 * q + 1], o = batch[3 * q + 2];
  const long long fixed = head ? o : s;
  for (int k = lane; k < d; k += 64) qvec[(size_t)q * d + k] = nodes[(size_t)fixed * d + k] * rel[(size_t)p * d + k];
  if (lane == 0 && pbias) {
    qb[2 * q] = pbias[p];
    qb[2 * q + 1] = head ? obias[o] : sbias[s];
  }
}

// four K-adjacent operand values of one row.  The address is clamped into the row and the tail (k >= d) is zeroed by
// mask_k4 at the point of USE: a select right after the load would make hipcc wait for the load there.
template <bool VEC>
__device__ __forceinline__ f32x4 load_k4(const float *__restrict__ row, int k, int d) {
  if (VEC) return *reinterpret_cast<const f32x4 *>(row + min(k, d - 4));   // d % 4 == 0: rows are 16-byte aligned
  f32x4 v;
#pragma unroll
  for (int c = 0; c < 4; ++c) v[c] = row[min(k + c, d - 1)];
  return v;
}
template <bool VEC>
__device__ __forceinline__ f32x4 mask_k4(f32x4 v, int k, int d) {
  if (VEC) return k < d ? v : f32x4{0.f, 0.f, 0.f, 0.f};                  // k < d implies k + 3 < d
#pragma unroll
  for (int c = 0; c < 4; ++c) v[c] = (k + c < d) ? v[c] : 0.f;
  return v;
}

// Same product with the operands staged through LDS: a workgroup owns 128 queries x 128 candidates (a 64 x 64 block
// per wave), every K step's two 128 x 16 operand slabs are fetched from L2 ONCE per workgroup (the register-only kernel
// fetches each slab twice, and 16 rows x 64 B per instruction is a poor shape for the L1), written to a double-buffered
// LDS tile (row stride 20 floats: the ds_read_b128 of 16 rows x 4 column groups is conflict-free) and read back as MFMA
// operands.  The loads of step t+1 are issued before the 64 MFMAs of step t and land in LDS after them.
constexpr int LDS_LD = 20;
template <bool VEC>
__global__ __launch_bounds__(WG) void score_all_lds_kernel(
    const float *__restrict__ qvec, const float *__restrict__ qb, const float *__restrict__ nodes,
    const float *__restrict__ cbias, float *__restrict__ scores, int Q, long long N, int d, int head, int q_blocks) {
  __shared__ __attribute__((aligned(16))) float sA[2][128 * LDS_LD], sB[2][128 * LDS_LD];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int i = lane & 15, kq = lane >> 4;
  const int qt = (blockIdx.x % q_blocks) * 128;
  const long long ct = (long long)(blockIdx.x / q_blocks) * 128;
  const int q0 = qt + (wave >> 1) * 64;
  const long long c0 = ct + (wave & 1) * 64;
  // staging: thread -> rows (tid >> 2) and (tid >> 2) + 64 of both slabs, 16-byte column group tid & 3
  const int sr = tid >> 2, sc = 4 * (tid & 3);
  const float *ga[2], *gb[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    ga[h] = qvec + (size_t)min(qt + sr + 64 * h, Q - 1) * d;
    gb[h] = nodes + (size_t)min(ct + sr + 64 * h, N - 1) * d;
  }
  f32x4 acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int steps = (d + 15) / 16;
  f32x4 sa[2], sb[2];
  auto fetch = [&](int t) {
    const int k = 16 * t + sc;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      sa[h] = load_k4<VEC>(ga[h], k, d);
      sb[h] = load_k4<VEC>(gb[h], k, d);
    }
  };
  auto stash = [&](int buf, int t) {         // zero the K tail here, so the compute loop never masks
    const int k = 16 * t + sc;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      *reinterpret_cast<f32x4 *>(&sA[buf][(sr + 64 * h) * LDS_LD + sc]) = mask_k4<VEC>(sa[h], k, d);
      *reinterpret_cast<f32x4 *>(&sB[buf][(sr + 64 * h) * LDS_LD + sc]) = mask_k4<VEC>(sb[h], k, d);
    }
  };
  fetch(0);
  stash(0, 0);
  __syncthreads();
  for (int t = 0; t < steps; ++t) {
    const int cur = t & 1;
    if (t + 1 < steps) fetch(t + 1);
    f32x4 av[4], bv[4];
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      av[a] = *reinterpret_cast<const f32x4 *>(&sA[cur][((wave >> 1) * 64 + 16 * a + i) * LDS_LD + 4 * kq]);
      bv[a] = *reinterpret_cast<const f32x4 *>(&sB[cur][((wave & 1) * 64 + 16 * a + i) * LDS_LD + 4 * kq]);
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b)
          acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[a][c], bv[b][c], acc[a][b], 0, 0, 0);
    __builtin_amdgcn_sched_barrier(0);
    if (t + 1 < steps) stash(cur ^ 1, t + 1);
    __syncthreads();
  }
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int qrow = q0 + 16 * a + 4 * kq + r;
      if (qrow >= Q) continue;
      float s1 = 0.f, s2 = 0.f;
      if (qb) { s1 = qb[2 * qrow]; s2 = qb[2 * qrow + 1]; }
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const long long col = c0 + 16 * b + i;
        if (col >= N) continue;
        float sc_ = acc[a][b][r];
        if (qb) {
          const float cb = cbias[col];
          sc_ += head ? ((cb + s1) + s2) : ((s2 + s1) + cb);
        }
        scores[(size_t)qrow * N + col] = sc_;
      }
    }
}

// ------------------------------------------------------------------ bf16 entity table
// The same product on v_mfma_f32_16x16x32_bf16.  The candidates are bf16 already; the query vector nodes[fixed] * rel[p] is an fp32
// number and is NOT rounded: it is written as three bf16 terms hi = rne(q), mid = rne(q - hi), lo = rne(q - hi - mid) whose sum is q
// exactly (24 significand bits = 3 x 8; the remainders are exact fp32 differences, formed with contraction off), and every bf16 x bf16 product is exact in fp32.  So the
// kernel adds the terms the fp32 evaluator adds on the widened table, in another order, at 3 of the 16x cheaper matrix instructions per
// 32 k instead of 8 fp32 ones per 32 k.
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// query terms [3][Q][dpad] (dpad = d rounded up to the K step of 32, the tail zeroed here: the product kernel loads whole 16-byte
// pieces of these rows without a clamp or a mask) and the query-side bias terms; one wave per query
__global__ __launch_bounds__(WG) void rank_query_bf16_kernel(
    const long long *__restrict__ batch, int Q, int head, const uint16_t *__restrict__ nodes,
    const float *__restrict__ rel, const float *__restrict__ sbias, const float *__restrict__ pbias,
    const float *__restrict__ obias, uint16_t *__restrict__ qs, float *__restrict__ qb, int d, int dpad) {
#pragma clang fp contract(off)
  const int q = blockIdx.x * (WG / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (q >= Q) return;
  const long long s = batch[3 * q], p = batch[3 * q + 1], o = batch[3 * q + 2];
  const long long fixed = head ? o : s;
  const size_t term = (size_t)Q * dpad;
  for (int k = lane; k < dpad; k += 64) {
    uint16_t hi = 0, mid = 0, lo = 0;
    if (k < d) {
      // the fp32 product as the fp32 evaluator forms it, then exact remainders: contraction is off in this function, a fused
      // fma(x, r, -hi) would split the unrounded product instead (closer to x r, but not what the fp32 kernel multiplies)
      const float v = bf16_widen(nodes[(size_t)fixed * d + k]) * rel[(size_t)p * d + k];
      hi = bf16_round(v);
      if (v - v == 0.f) {                                    // finite (an inf / NaN element is its own hi: mid = lo = 0)
        if ((hi & 0x7FFFu) == 0x7F80u) hi = (hi & 0x8000u) | 0x7F7Fu;     // |v| above the largest bf16 rounds to inf: take the largest bf16, the
        const float r1 = v - bf16_widen(hi);                              // remainder (same binade: exact) goes to mid and lo
        mid = bf16_round(r1);
        lo = bf16_round(r1 - bf16_widen(mid));
      }
    }
    uint16_t *dst = qs + (size_t)q * dpad + k;
    dst[0] = hi;
    dst[term] = mid;
    dst[2 * term] = lo;
  }
  if (lane == 0 && pbias) {
    qb[2 * q] = pbias[p];
    qb[2 * q + 1] = head ? obias[o] : sbias[s];
  }
}

// eight K-adjacent bf16 of one entity row (16 bytes); clamped into the row, the tail zeroed by mask_k8 at the point of use (as load_k4)
template <bool VEC>
__device__ __forceinline__ u32x4 load_k8(const uint16_t *__restrict__ row, int k, int d) {
  if (VEC) return *reinterpret_cast<const u32x4 *>(row + min(k, d - 8));   // d % 8 == 0: rows are 16-byte aligned
  u32x4 v;
#pragma unroll
  for (int c = 0; c < 4; ++c) v[c] = (unsigned)row[min(k + 2 * c, d - 1)] | ((unsigned)row[min(k + 2 * c + 1, d - 1)] << 16);
  return v;
}
template <bool VEC>
__device__ __forceinline__ u32x4 mask_k8(u32x4 v, int k, int d) {
  if (VEC) return k < d ? v : u32x4{0u, 0u, 0u, 0u};                       // k < d implies k + 7 < d
#pragma unroll
  for (int c = 0; c < 4; ++c) v[c] &= (k + 2 * c < d ? 0x0000FFFFu : 0u) | (k + 2 * c + 1 < d ? 0xFFFF0000u : 0u);
  return v;
}

// The shape of score_all_lds_kernel: 128 queries x 128 candidates per workgroup, 64 x 64 per wave, double-buffered LDS slabs, the loads
// of step t + 1 issued before the MFMAs of step t.  A K step is 32: a slab row is 32 bf16 = 64 bytes = four 16-byte pieces, lane
// 16 kq + i reads piece kq of row i (the operand map of v_mfma_f32_16x16x32_bf16: A[row l & 15][k = 8 (l >> 4) + j], B likewise by column)
// and uses each of its four B fragments against the hi, mid and lo A fragments: 48 MFMAs per step and wave behind 16 ds_read_b128.
// LDS rows are NOT padded: piece c of row r sits at piece c ^ ((r >> 2) & 2) of its 64 bytes.  A ds_read_b128 is served in four groups of
// 16 lanes that hold all 16 rows i, with piece a on rows 0-3 and 12-15 and piece a ^ 1 on rows 4-11; rows i, i + 4, i + 8, i + 12 share a
// 256-byte bank row, and with the swizzle they take pieces a, a ^ 1, a ^ 3, a ^ 2 of it: all distinct, no conflict.
constexpr int SLAB = 128 * 32;          // bf16 elements of one 128-row slab
__device__ __forceinline__ int slab_at(int row, int piece) { return row * 32 + 8 * (piece ^ ((row >> 2) & 2)); }

template <bool VEC>
__global__ __launch_bounds__(WG) void score_all_bf16_kernel(
    const uint16_t *__restrict__ qs, const float *__restrict__ qb, const uint16_t *__restrict__ nodes,
    const float *__restrict__ cbias, float *__restrict__ scores, int Q, long long N, int d, int dpad, int head, int q_blocks) {
  __shared__ __attribute__((aligned(16))) uint16_t sA[2][3][SLAB], sB[2][SLAB];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int i = lane & 15, kq = lane >> 4;
  const int qt = (blockIdx.x % q_blocks) * 128;
  const long long ct = (long long)(blockIdx.x / q_blocks) * 128;
  const int q0 = qt + (wave >> 1) * 64;
  const long long c0 = ct + (wave & 1) * 64;
  // staging: thread -> rows (tid >> 2) and (tid >> 2) + 64 of the four slabs, 16-byte piece tid & 3
  const int sr = tid >> 2, sc = tid & 3;
  const size_t term = (size_t)Q * dpad;
  const uint16_t *ga[2], *gb[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    ga[h] = qs + (size_t)min(qt + sr + 64 * h, Q - 1) * dpad;
    gb[h] = nodes + (size_t)min(ct + sr + 64 * h, N - 1) * d;
  }
  f32x4 acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int steps = dpad / 32;
  u32x4 sa[3][2], sb[2];
  auto fetch = [&](int t) {
    const int k = 32 * t + 8 * sc;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
#pragma unroll
      for (int m = 0; m < 3; ++m) sa[m][h] = *reinterpret_cast<const u32x4 *>(ga[h] + m * term + k);   // k + 7 < dpad, zero past d
      sb[h] = load_k8<VEC>(gb[h], k, d);
    }
  };
  auto stash = [&](int buf, int t) {         // zero the K tail of the entity rows here, so the compute loop never masks
    const int k = 32 * t + 8 * sc;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int at = slab_at(sr + 64 * h, sc);
#pragma unroll
      for (int m = 0; m < 3; ++m) *reinterpret_cast<u32x4 *>(&sA[buf][m][at]) = sa[m][h];
      *reinterpret_cast<u32x4 *>(&sB[buf][at]) = mask_k8<VEC>(sb[h], k, d);
    }
  };
  fetch(0);
  stash(0, 0);
  __syncthreads();
  for (int t = 0; t < steps; ++t) {
    const int cur = t & 1;
    if (t + 1 < steps) fetch(t + 1);
    bf16x8 av[3][4], bv[4];
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      const int ra = slab_at((wave >> 1) * 64 + 16 * a + i, kq), rb = slab_at((wave & 1) * 64 + 16 * a + i, kq);
#pragma unroll
      for (int m = 0; m < 3; ++m) av[m][a] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4 *>(&sA[cur][m][ra]));
      bv[a] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4 *>(&sB[cur][rb]));
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int m = 2; m >= 0; --m)             // lo, mid, hi: the small terms first
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b)
          acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av[m][a], bv[b], acc[a][b], 0, 0, 0);
    __builtin_amdgcn_sched_barrier(0);
    if (t + 1 < steps) stash(cur ^ 1, t + 1);
    __syncthreads();
  }
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int qrow = q0 + 16 * a + 4 * kq + r;
      if (qrow >= Q) continue;
      float s1 = 0.f, s2 = 0.f;
      if (qb) { s1 = qb[2 * qrow]; s2 = qb[2 * qrow + 1]; }
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const long long col = c0 + 16 * b + i;
        if (col >= N) continue;
        float sc_ = acc[a][b][r];
        if (qb) {
          const float cb = cbias[col];
          sc_ += head ? ((cb + s1) + s2) : ((s2 + s1) + cb);
        }
        scores[(size_t)qrow * N + col] = sc_;
      }
    }
}

__global__ void rank_filter_kernel(float *__restrict__ scores, long long N, const int *__restrict__ fq,
                                   const int *__restrict__ fn, long long F) {
  for (long long e = (long long)blockIdx.x * WG + threadIdx.x; e < F; e += (long long)gridDim.x * WG)
    scores[(size_t)fq[e] * N + fn[e]] = -INFINITY;
}

// one workgroup per query: #scores above the target's and #scores equal to it (the target included)
__global__ __launch_bounds__(WG) void rank_count_kernel(const float *__restrict__ scores,
                                                        const long long *__restrict__ batch, int head, long long N,
                                                        long long *__restrict__ greater, long long *__restrict__ ties) {
  __shared__ int red[2 * (WG / 64)];
  const int q = blockIdx.x;
  const float *row = scores + (size_t)q * N;
  const float t = row[batch[3 * q + (head ? 0 : 2)]];
  int g = 0, e = 0;
  for (long long n = threadIdx.x; n < N; n += WG) {
    const float s = row[n];
    g += s > t;
    e += s == t;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    g += __shfl_down(g, off);
    e += __shfl_down(e, off);
  }
  if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6] = g; red[WG / 64 + (threadIdx.x >> 6)] = e; }
  __syncthreads();
  if (threadIdx.x == 0) {
    long long gs = 0, es = 0;
    for (int w = 0; w < WG / 64; ++w) { gs += red[w]; es += red[WG / 64 + w]; }
    greater[q] = gs;
    ties[q] = es;
  }
}

}  // namespace

extern "C" int rgcn_distmult_score_all_f32(const int64_t *batch, int64_t Q, int32_t head, const float *nodes,
                                           const float *rel, const float *sbias, const float *pbias,
                                           const float *obias, float *qvec, float *qbias, float *scores,
                                           int64_t n_nodes, int32_t n_rel, int32_t d, void *stream) {
  (void)n_rel;
  if (Q < 0 || n_nodes <= 0 || d <= 0 || Q > INT32_MAX || (Q && (!batch || !nodes || !rel || !qvec || !scores))) {
    rgcn_set_error("distmult_score_all: bad argument");
    return RGCN_EINVAL;
  }
  if ((sbias != nullptr) != (pbias != nullptr) || (sbias != nullptr) != (obias != nullptr) || (sbias && !qbias)) {
    rgcn_set_error("distmult_score_all: biases must be all set (with the qbias scratch) or all NULL");
    return RGCN_EINVAL;
  }
  if (Q == 0) return RGCN_OK;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(rank_query_kernel, dim3((unsigned)((Q + 3) / 4)), dim3(WG), 0, st,
                     reinterpret_cast<const long long *>(batch), (int)Q, head, nodes, rel, sbias, pbias, obias, qvec,
                     qbias, d);
  {     // (round 5: the register-only tile variants behind RGCN_RANK_TILE -- measured slower than this LDS-staged kernel in round 1 -- are gone)
    const int qbl = (int)((Q + 127) / 128);
    const int64_t nwg = ((n_nodes + 127) / 128) * qbl;
    if (nwg > INT32_MAX) { rgcn_set_error("distmult_score_all: too many scores in one call; split the batch"); return RGCN_EUNSUPPORTED; }
    const float *qb1 = sbias ? qbias : nullptr, *cb1 = sbias ? (head ? sbias : obias) : nullptr;
    if (d % 4 == 0)
      hipLaunchKernelGGL(score_all_lds_kernel<true>, dim3((unsigned)nwg), dim3(WG), 0, st, qvec, qb1, nodes, cb1, scores,
                         (int)Q, (long long)n_nodes, d, head, qbl);
    else
      hipLaunchKernelGGL(score_all_lds_kernel<false>, dim3((unsigned)nwg), dim3(WG), 0, st, qvec, qb1, nodes, cb1, scores,
                         (int)Q, (long long)n_nodes, d, head, qbl);
    HIP_TRY(hipGetLastError());
    return RGCN_OK;
  }
}

static int64_t k_pad32(int32_t d) { return ((int64_t)d + 31) / 32 * 32; }

extern "C" int64_t rgcn_distmult_score_all_bf16_workspace_bytes(int64_t Q, int32_t d) {
  return (Q < 0 || d <= 0) ? 0 : 3 * Q * k_pad32(d) * (int64_t)sizeof(uint16_t);
}

extern "C" int rgcn_distmult_score_all_bf16(const int64_t *batch, int64_t Q, int32_t head, const uint16_t *nodes,
                                            const float *rel, const float *sbias, const float *pbias,
                                            const float *obias, uint16_t *qsplit, float *qbias, float *scores,
                                            int64_t n_nodes, int32_t n_rel, int32_t d, void *stream) {
  (void)n_rel;
  if (Q < 0 || n_nodes <= 0 || d <= 0 || Q > INT32_MAX || (Q && (!batch || !nodes || !rel || !qsplit || !scores)) ||
      (reinterpret_cast<uintptr_t>(qsplit) & 15)) {
    rgcn_set_error("distmult_score_all_bf16: bad argument (qsplit: 16-byte aligned)");
    return RGCN_EINVAL;
  }
  if ((sbias != nullptr) != (pbias != nullptr) || (sbias != nullptr) != (obias != nullptr) || (sbias && !qbias)) {
    rgcn_set_error("distmult_score_all_bf16: biases must be all set (with the qbias scratch) or all NULL");
    return RGCN_EINVAL;
  }
  if (Q == 0) return RGCN_OK;
  const int qbl = (int)((Q + 127) / 128);
  const int64_t nwg = ((n_nodes + 127) / 128) * qbl;
  if (nwg > INT32_MAX) { rgcn_set_error("distmult_score_all_bf16: too many scores in one call; split the batch"); return RGCN_EUNSUPPORTED; }
  hipStream_t st = (hipStream_t)stream;
  const int dpad = (int)k_pad32(d);
  hipLaunchKernelGGL(rank_query_bf16_kernel, dim3((unsigned)((Q + 3) / 4)), dim3(WG), 0, st,
                     reinterpret_cast<const long long *>(batch), (int)Q, head, nodes, rel, sbias, pbias, obias, qsplit,
                     qbias, d, dpad);
  const float *qb1 = sbias ? qbias : nullptr, *cb1 = sbias ? (head ? sbias : obias) : nullptr;
  // 16-byte loads of the entity rows: d % 8 == 0 on an aligned table (WN18, FB15k-237); else element by element
  if (d % 8 == 0 && (reinterpret_cast<uintptr_t>(nodes) & 15) == 0)
    hipLaunchKernelGGL(score_all_bf16_kernel<true>, dim3((unsigned)nwg), dim3(WG), 0, st, qsplit, qb1, nodes, cb1, scores,
                       (int)Q, (long long)n_nodes, d, dpad, head, qbl);
  else
    hipLaunchKernelGGL(score_all_bf16_kernel<false>, dim3((unsigned)nwg), dim3(WG), 0, st, qsplit, qb1, nodes, cb1, scores,
                       (int)Q, (long long)n_nodes, d, dpad, head, qbl);
  HIP_TRY(hipGetLastError());
  return RGCN_OK;
}

extern "C" int rgcn_rank_filter_f32(float *scores, int64_t Q, int64_t n_nodes, const int32_t *filt_q,
                                    const int32_t *filt_n, int64_t F, void *stream) {
  if (Q < 0 || n_nodes <= 0 || F < 0 || (F && (!scores || !filt_q || !filt_n))) {
    rgcn_set_error("rank_filter: bad argument");
    return RGCN_EINVAL;
  }
  if (F == 0) return RGCN_OK;
  hipLaunchKernelGGL(rank_filter_kernel, dim3((unsigned)std::min<int64_t>((F + WG - 1) / WG, 1 << 16)), dim3(WG), 0,
                     (hipStream_t)stream, scores, (long long)n_nodes, filt_q, filt_n, (long long)F);
  HIP_TRY(hipGetLastError());
  return RGCN_OK;
}

extern "C" int rgcn_rank_count_f32(const float *scores, const int64_t *batch, int64_t Q, int32_t head,
                                   int64_t n_nodes, int64_t *greater, int64_t *ties, void *stream) {
  if (Q < 0 || n_nodes <= 0 || Q > INT32_MAX || (Q && (!scores || !batch || !greater || !ties))) {
    rgcn_set_error("rank_count: bad argument");
    return RGCN_EINVAL;
  }
  if (Q == 0) return RGCN_OK;
  hipLaunchKernelGGL(rank_count_kernel, dim3((unsigned)Q), dim3(WG), 0, (hipStream_t)stream, scores,
                     reinterpret_cast<const long long *>(batch), head, (long long)n_nodes,
                     reinterpret_cast<long long *>(greater), reinterpret_cast<long long *>(ties));
  HIP_TRY(hipGetLastError());
  return RGCN_OK;
}
