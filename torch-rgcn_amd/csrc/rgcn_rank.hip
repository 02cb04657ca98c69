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
// Second route (rgcn_distmult_rank_fused_*, utils/misc.py:40-58, 71-99): the same tile product with an epilogue that compares every score
// with the target's instead of storing it -- greater / ties per query without a [Q, N] buffer.
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

// The product loop of one 128 x 128 tile, shared by score_all_lds_kernel and the fused evaluator's target and count kernels
// (rank_target_kernel, rank_count_fused_kernel): whoever instantiates it gets the same K permutation and the same MFMA chain per
// accumulator, hence the same bits for the same pair of rows wherever the pair sits in a tile.  ga / gb: this thread's two staging rows
// (tid >> 2 and + 64) of the query and the candidate slab.  Ends on a barrier: the LDS slabs may be refilled right away.
template <bool VEC>
__device__ __forceinline__ void tile_product_f32(const float *const (&ga)[2], const float *const (&gb)[2], int d,
                                                 float (&sA)[2][128 * LDS_LD], float (&sB)[2][128 * LDS_LD], f32x4 (&acc)[4][4]) {
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int i = lane & 15, kq = lane >> 4;
  // staging: thread -> rows (tid >> 2) and (tid >> 2) + 64 of both slabs, 16-byte column group tid & 3
  const int sr = tid >> 2, sc = 4 * (tid & 3);
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
}

// The epilogue of a wave's 64 x 64 block, shared like the product (fp32 and bf16 tiles hold their accumulators alike): the parenthesised
// bias sum on every cell with qrow < Q and col < n_cols.  row(a * 4 + r, qrow) opens a query row and returns its state; cb_of(col) is the
// candidate-side bias of a column; cell(state, a * 4 + r, b, col, score) takes the finished score.
template <class Row, class CB, class Cell>
__device__ __forceinline__ void tile_epilogue(const f32x4 (&acc)[4][4], int q0, long long c0, int Q, long long n_cols,
                                              const float *__restrict__ qb, int head, Row row, CB cb_of, Cell cell) {
  const int lane = threadIdx.x & 63, i = lane & 15, kq = lane >> 4;
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int qrow = q0 + 16 * a + 4 * kq + r;
      if (qrow >= Q) continue;
      float s1 = 0.f, s2 = 0.f;
      if (qb) { s1 = qb[2 * qrow]; s2 = qb[2 * qrow + 1]; }
      auto st = row(a * 4 + r, qrow);
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const long long col = c0 + 16 * b + i;
        if (col >= n_cols) continue;
        float sc_ = acc[a][b][r];
        if (qb) {
          const float cb = cb_of(col);
          sc_ += head ? ((cb + s1) + s2) : ((s2 + s1) + cb);
        }
        cell(st, a * 4 + r, b, col, sc_);
      }
    }
}

template <bool VEC>
__global__ __launch_bounds__(WG) void score_all_lds_kernel(
    const float *__restrict__ qvec, const float *__restrict__ qb, const float *__restrict__ nodes,
    const float *__restrict__ cbias, float *__restrict__ scores, int Q, long long N, int d, int head, int q_blocks) {
  __shared__ __attribute__((aligned(16))) float sA[2][128 * LDS_LD], sB[2][128 * LDS_LD];
  const int tid = threadIdx.x, wave = tid >> 6;
  const int qt = (blockIdx.x % q_blocks) * 128;
  const long long ct = (long long)(blockIdx.x / q_blocks) * 128;
  const int sr = tid >> 2;
  const float *ga[2], *gb[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    ga[h] = qvec + (size_t)min(qt + sr + 64 * h, Q - 1) * d;
    gb[h] = nodes + (size_t)min(ct + sr + 64 * h, N - 1) * d;
  }
  f32x4 acc[4][4];
  tile_product_f32<VEC>(ga, gb, d, sA, sB, acc);
  tile_epilogue(acc, qt + (wave >> 1) * 64, ct + (wave & 1) * 64, Q, N, qb, head,
                [&](int, int qrow) { return scores + (size_t)qrow * N; },
                [&](long long col) { return cbias[col]; },
                [&](float *out, int, int, long long col, float sc_) { out[col] = sc_; });
}

// ------------------------------------------------------------------ fused evaluator: ranks without the score matrix
// Pass 2: tscore[q] = the score of query q's own target, from the SAME product and epilogue as score_all -- one 128 x 128 tile per
// block of 128 queries whose "candidate" row j is nodes[target of query qt + j]; the diagonal cells are kept.
__device__ __forceinline__ long long rank_target(const long long *__restrict__ batch, int q, int head) { return batch[3 * q + (head ? 0 : 2)]; }

template <bool VEC>
__global__ __launch_bounds__(WG) void rank_target_kernel(
    const float *__restrict__ qvec, const float *__restrict__ qb, const float *__restrict__ nodes, const float *__restrict__ cbias,
    const long long *__restrict__ batch, float *__restrict__ tscore, int Q, int d, int head) {
  __shared__ __attribute__((aligned(16))) float sA[2][128 * LDS_LD], sB[2][128 * LDS_LD];
  const int tid = threadIdx.x, wave = tid >> 6;
  const int qt = blockIdx.x * 128;
  const int sr = tid >> 2;
  const float *ga[2], *gb[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int q = min(qt + sr + 64 * h, Q - 1);
    ga[h] = qvec + (size_t)q * d;
    gb[h] = nodes + (size_t)rank_target(batch, q, head) * d;
  }
  f32x4 acc[4][4];
  tile_product_f32<VEC>(ga, gb, d, sA, sB, acc);
  tile_epilogue(acc, qt + (wave >> 1) * 64, (long long)qt + (wave & 1) * 64, Q, (long long)Q, qb, head,
                [&](int, int qrow) { return qrow; },
                [&](long long col) { return cbias[rank_target(batch, (int)col, head)]; },
                [&](int qrow, int, int, long long col, float sc_) { if (col == qrow) tscore[qrow] = sc_; });
}

// Pass 3's epilogue: the cells of one tile compared with their query's target score instead of stored.  mask: the filter bits
// [Q][mask_w] (NULL = raw ranks), one word per 32 candidates -- the lane's four columns c0 + 16 b + i (c0 a multiple of 64) sit in words
// c0 / 32 and c0 / 32 + 1.  A filtered cell compares as -inf, which is what rank_filter_kernel writes into the score matrix of the
// materialised route.  Counters: a lane's 16 rows would cost 32 registers across the product loop; instead every row's (greater, equal)
// of this tile -- at most 64 each, packed in one word -- is summed over the 16 lanes that share the row (four DPP steps) and kept by
// lane i = row: g / e hold the counts of row 16 (i >> 2) + 4 kq + (i & 3) of the wave's 64.
struct RankRow { float t; unsigned w[2]; };

__device__ __forceinline__ void tile_count(const f32x4 (&acc)[4][4], int q0, long long c0, int Q, long long N, const float *__restrict__ qb,
                                           const float *__restrict__ cbias, int head, const float *__restrict__ tscore,
                                           const unsigned *__restrict__ mask, long long mask_w, int &g, int &e) {
  const int i = threadIdx.x & 15;
  int c[16];
#pragma unroll
  for (int row = 0; row < 16; ++row) c[row] = 0;
  tile_epilogue(acc, q0, c0, Q, N, qb, head,
                [&](int, int qrow) {
                  RankRow st{tscore[qrow], {0u, 0u}};
                  if (mask) {
                    const long long w0 = c0 >> 5;
                    const unsigned *mrow = mask + (size_t)qrow * mask_w;
                    if (w0 < mask_w) st.w[0] = mrow[w0];                  // (the right half of a ragged last tile may start past N)
                    if (w0 + 1 < mask_w) st.w[1] = mrow[w0 + 1];
                  }
                  return st;
                },
                [&](long long col) { return cbias[col]; },
                [&](const RankRow &st, int row, int b, long long, float sc_) {
                  const float s = (st.w[b >> 1] >> (16 * (b & 1) + i)) & 1u ? -INFINITY : sc_;
                  c[row] += (s > st.t) + ((s == st.t) << 16);
                });
#pragma unroll
  for (int row = 0; row < 16; ++row) {
    int v = c[row];
    v += dpp_i<0xB1>(v, v);        // quad_perm [1,0,3,2]
    v += dpp_i<0x4E>(v, v);        // quad_perm [2,3,0,1]
    v += dpp_i<0x141>(v, v);       // row_half_mirror
    v += dpp_i<0x140>(v, v);       // row_mirror: every lane of the 16 holds the row's sum
    g += i == row ? v & 0xFFFF : 0;
    e += i == row ? v >> 16 : 0;
  }
}

// strip s of `strips` owns the candidate tiles [s n_tiles / strips, (s + 1) n_tiles / strips): sizes differ by one at most, and a strip
// beyond the tiles owns none
__device__ __forceinline__ long long strip_first(long long s, long long n_tiles, int strips) { return s * n_tiles / strips; }

// a wave's counters -> partial[2 strip + candidate half of the wave][q] = (greater, equal)
__device__ __forceinline__ void strip_store(int g, int e, int q0, int Q, uint2 *__restrict__ part) {
  const int lane = threadIdx.x & 63, i = lane & 15, kq = lane >> 4;
  const int qrow = q0 + 16 * (i >> 2) + 4 * kq + (i & 3);
  if (qrow < Q) part[qrow] = uint2{(unsigned)g, (unsigned)e};
}

// Pass 3: a workgroup owns one block of 128 queries and a strip of candidate tiles; counters stay in registers over the strip.
template <bool VEC>
__global__ __launch_bounds__(WG) void rank_count_fused_kernel(
    const float *__restrict__ qvec, const float *__restrict__ qb, const float *__restrict__ nodes, const float *__restrict__ cbias,
    const float *__restrict__ tscore, const unsigned *__restrict__ mask, long long mask_w, uint2 *__restrict__ partial,
    int Q, long long N, int d, int head, int q_blocks, int strips) {
  __shared__ __attribute__((aligned(16))) float sA[2][128 * LDS_LD], sB[2][128 * LDS_LD];
  const int tid = threadIdx.x, wave = tid >> 6;
  const int qt = (blockIdx.x % q_blocks) * 128, strip = blockIdx.x / q_blocks;
  const long long n_tiles = (N + 127) / 128;
  const long long tile_end = strip_first(strip + 1, n_tiles, strips);
  const int sr = tid >> 2, q0 = qt + (wave >> 1) * 64;
  const float *ga[2], *gb[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) ga[h] = qvec + (size_t)min(qt + sr + 64 * h, Q - 1) * d;
  int g = 0, e = 0;
  for (long long tile = strip_first(strip, n_tiles, strips); tile < tile_end; ++tile) {
    const long long ct = tile * 128;
#pragma unroll
    for (int h = 0; h < 2; ++h) gb[h] = nodes + (size_t)min(ct + sr + 64 * h, N - 1) * d;
    f32x4 acc[4][4];
    tile_product_f32<VEC>(ga, gb, d, sA, sB, acc);
    // the rows' target scores, bias terms and addresses are formed again for every tile: hoisted out of this loop they would sit in
    // ~100 registers through the product, and the kernel would drop to one workgroup per compute unit
    int q0t = q0;
    asm volatile("" : "+v"(q0t));
    tile_count(acc, q0t, ct + (wave & 1) * 64, Q, N, qb, cbias, head, tscore, mask, mask_w, g, e);
  }
  strip_store(g, e, q0, Q, partial + (size_t)(2 * strip + (wave & 1)) * Q);
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

// The bf16 product loop of one tile, shared by score_all_bf16_kernel, rank_target_bf16_kernel and rank_count_fused_bf16_kernel (as
// tile_product_f32: same lo-mid-hi order and MFMA chain per accumulator for whoever instantiates it).  ga: this thread's two staging rows
// of the hi term (mid and lo `term` elements further on), gb: of the candidate slab.  Ends on a barrier.
template <bool VEC>
__device__ __forceinline__ void tile_product_bf16(const uint16_t *const (&ga)[2], const uint16_t *const (&gb)[2], size_t term, int d, int dpad,
                                                  uint16_t (&sA)[2][3][SLAB], uint16_t (&sB)[2][SLAB], f32x4 (&acc)[4][4]) {
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int i = lane & 15, kq = lane >> 4;
  // staging: thread -> rows (tid >> 2) and (tid >> 2) + 64 of the four slabs, 16-byte piece tid & 3
  const int sr = tid >> 2, sc = tid & 3;
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
}

template <bool VEC>
__global__ __launch_bounds__(WG) void score_all_bf16_kernel(
    const uint16_t *__restrict__ qs, const float *__restrict__ qb, const uint16_t *__restrict__ nodes,
    const float *__restrict__ cbias, float *__restrict__ scores, int Q, long long N, int d, int dpad, int head, int q_blocks) {
  __shared__ __attribute__((aligned(16))) uint16_t sA[2][3][SLAB], sB[2][SLAB];
  const int tid = threadIdx.x, wave = tid >> 6;
  const int qt = (blockIdx.x % q_blocks) * 128;
  const long long ct = (long long)(blockIdx.x / q_blocks) * 128;
  const int sr = tid >> 2;
  const uint16_t *ga[2], *gb[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    ga[h] = qs + (size_t)min(qt + sr + 64 * h, Q - 1) * dpad;
    gb[h] = nodes + (size_t)min(ct + sr + 64 * h, N - 1) * d;
  }
  f32x4 acc[4][4];
  tile_product_bf16<VEC>(ga, gb, (size_t)Q * dpad, d, dpad, sA, sB, acc);
  tile_epilogue(acc, qt + (wave >> 1) * 64, ct + (wave & 1) * 64, Q, N, qb, head,
                [&](int, int qrow) { return scores + (size_t)qrow * N; },
                [&](long long col) { return cbias[col]; },
                [&](float *out, int, int, long long col, float sc_) { out[col] = sc_; });
}

// the fused evaluator's passes 2 and 3 on the bf16 table (see rank_target_kernel, rank_count_fused_kernel)
template <bool VEC>
__global__ __launch_bounds__(WG) void rank_target_bf16_kernel(
    const uint16_t *__restrict__ qs, const float *__restrict__ qb, const uint16_t *__restrict__ nodes, const float *__restrict__ cbias,
    const long long *__restrict__ batch, float *__restrict__ tscore, int Q, int d, int dpad, int head) {
  __shared__ __attribute__((aligned(16))) uint16_t sA[2][3][SLAB], sB[2][SLAB];
  const int tid = threadIdx.x, wave = tid >> 6;
  const int qt = blockIdx.x * 128;
  const int sr = tid >> 2;
  const uint16_t *ga[2], *gb[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int q = min(qt + sr + 64 * h, Q - 1);
    ga[h] = qs + (size_t)q * dpad;
    gb[h] = nodes + (size_t)rank_target(batch, q, head) * d;
  }
  f32x4 acc[4][4];
  tile_product_bf16<VEC>(ga, gb, (size_t)Q * dpad, d, dpad, sA, sB, acc);
  tile_epilogue(acc, qt + (wave >> 1) * 64, (long long)qt + (wave & 1) * 64, Q, (long long)Q, qb, head,
                [&](int, int qrow) { return qrow; },
                [&](long long col) { return cbias[rank_target(batch, (int)col, head)]; },
                [&](int qrow, int, int, long long col, float sc_) { if (col == qrow) tscore[qrow] = sc_; });
}

template <bool VEC>
__global__ __launch_bounds__(WG) void rank_count_fused_bf16_kernel(
    const uint16_t *__restrict__ qs, const float *__restrict__ qb, const uint16_t *__restrict__ nodes, const float *__restrict__ cbias,
    const float *__restrict__ tscore, const unsigned *__restrict__ mask, long long mask_w, uint2 *__restrict__ partial,
    int Q, long long N, int d, int dpad, int head, int q_blocks, int strips) {
  __shared__ __attribute__((aligned(16))) uint16_t sA[2][3][SLAB], sB[2][SLAB];
  const int tid = threadIdx.x, wave = tid >> 6;
  const int qt = (blockIdx.x % q_blocks) * 128, strip = blockIdx.x / q_blocks;
  const long long n_tiles = (N + 127) / 128;
  const long long tile_end = strip_first(strip + 1, n_tiles, strips);
  const int sr = tid >> 2, q0 = qt + (wave >> 1) * 64;
  const uint16_t *ga[2], *gb[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) ga[h] = qs + (size_t)min(qt + sr + 64 * h, Q - 1) * dpad;
  int g = 0, e = 0;
  for (long long tile = strip_first(strip, n_tiles, strips); tile < tile_end; ++tile) {
    const long long ct = tile * 128;
#pragma unroll
    for (int h = 0; h < 2; ++h) gb[h] = nodes + (size_t)min(ct + sr + 64 * h, N - 1) * d;
    f32x4 acc[4][4];
    tile_product_bf16<VEC>(ga, gb, (size_t)Q * dpad, d, dpad, sA, sB, acc);
    // the rows' target scores, bias terms and addresses are formed again for every tile: hoisted out of this loop they would sit in
    // ~100 registers through the product, and the kernel would drop to one workgroup per compute unit
    int q0t = q0;
    asm volatile("" : "+v"(q0t));
    tile_count(acc, q0t, ct + (wave & 1) * 64, Q, N, qb, cbias, head, tscore, mask, mask_w, g, e);
  }
  strip_store(g, e, q0, Q, partial + (size_t)(2 * strip + (wave & 1)) * Q);
}

// ------------------------------------------------------------------ top-k prediction: the k best candidates per query
// The product and epilogue of score_all again, with an epilogue that SELECTS.  Selection is integer max-selection on 64-bit keys:
//   high word = the score's order-preserving unsigned image (-0 canonicalised to +0, then: negative -> all bits flipped, else sign set),
//   low word  = ~id, so that among equal scores the lower id is the larger key.
// Keys of one query are distinct (ids are) and never 0 (id < 2^31 sets the low word's top bit): 0 marks an empty slot, and "score
// descending, id ascending" is "key descending" -- one answer whatever the strips, the tile a candidate sits in or the insertion order.
// A filtered cell, a cell out of range and a score of -inf (what a filtered cell holds on the materialised route) produce no key.
// NaN scores are outside the contract (a NaN lands wherever its bit pattern puts it).
constexpr int TOPK_MAX = 32;

__device__ __forceinline__ unsigned long long topk_key(float s, unsigned id) {
  unsigned b = __float_as_uint(s);
  b = b == 0x80000000u ? 0u : b;
  b = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
  return ((unsigned long long)b << 32) | (unsigned)~id;
}

// LDS words of a wave's lists: other lanes of the wave write them between one lane's reads, so every access is a relaxed atomic (a plain
// load may be kept in a register across the insertion loop); the wave's LDS operations execute in program order
__device__ __forceinline__ unsigned long long lds_ld64(const unsigned long long *p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ void lds_st64(unsigned long long *p, unsigned long long v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// 64-bit values over the 16 lanes of a DPP row (all of them active): after the four exchanges every lane holds the row's result
template <int CTRL>
__device__ __forceinline__ unsigned long long dpp_u64(unsigned long long v) {
  const unsigned lo = (unsigned)dpp_i<CTRL>((int)(unsigned)v, (int)(unsigned)v);
  const unsigned hi = (unsigned)dpp_i<CTRL>((int)(unsigned)(v >> 32), (int)(unsigned)(v >> 32));
  return ((unsigned long long)hi << 32) | lo;
}
__device__ __forceinline__ unsigned long long row16_max(unsigned long long v) {
  unsigned long long o;
  o = dpp_u64<0xB1>(v); v = o > v ? o : v;         // quad_perm [1,0,3,2]
  o = dpp_u64<0x4E>(v); v = o > v ? o : v;         // quad_perm [2,3,0,1]
  o = dpp_u64<0x141>(v); v = o > v ? o : v;        // row_half_mirror
  o = dpp_u64<0x140>(v); v = o > v ? o : v;        // row_mirror
  return v;
}
__device__ __forceinline__ unsigned long long row16_min(unsigned long long v) {
  unsigned long long o;
  o = dpp_u64<0xB1>(v); v = o < v ? o : v;
  o = dpp_u64<0x4E>(v); v = o < v ? o : v;
  o = dpp_u64<0x141>(v); v = o < v ? o : v;
  o = dpp_u64<0x140>(v); v = o < v ? o : v;
  return v;
}
__device__ __forceinline__ int row16_min_i(int v) {
  v = min(v, dpp_i<0xB1>(v, v));
  v = min(v, dpp_i<0x4E>(v, v));
  v = min(v, dpp_i<0x141>(v, v));
  v = min(v, dpp_i<0x140>(v, v));
  return v;
}

// One query row of a tile: the 16 lanes that share it (one DPP row, all of them active) hold up to four keys each that beat the row's
// threshold `thr` = the smallest of the row's k kept keys (an empty slot is 0, the smallest; 0 = no key).  They are inserted one per turn,
// the row's LARGEST pending key first -- the threshold rises as fast as it can, and after k turns at most nothing is left that beats it.
// A turn is cooperative: lane i holds slots i and i + 16 of the list, the first slot equal to thr is replaced, and the new threshold is
// the minimum over the lanes' slots -- no lane walks the list.  The four rows of a wave instruction take their turns side by side, every
// step is predicated (no DPP under a branch), and the loop ends when no row of the wave has a key left.
__device__ __forceinline__ void topk_insert(unsigned long long (&pend)[4], unsigned long long *list, unsigned long long *thr_p, int k,
                                            unsigned long long thr) {
  const int i = threadIdx.x & 15;
  for (;;) {
    unsigned long long m = pend[0] > pend[1] ? pend[0] : pend[1];
    const unsigned long long m2 = pend[2] > pend[3] ? pend[2] : pend[3];
    m = m > m2 ? m : m2;
    m = m > thr ? m : 0ull;
    if (!__builtin_amdgcn_ballot_w64(m != 0ull)) break;
    const unsigned long long gm = row16_max(m);
    const bool go = gm != 0ull;                                  // the same for the 16 lanes of the row
    unsigned long long e0 = i < k ? lds_ld64(list + i) : ~0ull;
    unsigned long long e1 = i + 16 < k ? lds_ld64(list + (i + 16)) : ~0ull;
    const int at = row16_min_i(e0 == thr ? i : (e1 == thr ? i + 16 : 64));
    if (go && at == i) { e0 = gm; lds_st64(list + i, gm); }
    if (go && at == i + 16) { e1 = gm; lds_st64(list + (i + 16), gm); }
    const unsigned long long low = row16_min(e0 < e1 ? e0 : e1);
    thr = go ? low : thr;
    if (go && i == 0) lds_st64(thr_p, thr);
    pend[0] = pend[0] == gm ? 0ull : pend[0];
    pend[1] = pend[1] == gm ? 0ull : pend[1];
    pend[2] = pend[2] == gm ? 0ull : pend[2];
    pend[3] = pend[3] == gm ? 0ull : pend[3];
  }
}

// The selecting epilogue of one tile: tile_epilogue over the wave's whole 64 x 64 block (n_cols = c0 + 64, so that no lane leaves the
// cell loop and the 16 lanes of a row stay together; a column past N is clamped for its bias and produces no key).  Thresholds, lists and
// mask words are read again for every tile: nothing of a row lives in registers across the product loop.
struct TopkRow { unsigned long long thr; unsigned w[2]; int lr; };

__device__ __forceinline__ void tile_select(const f32x4 (&acc)[4][4], int q0, long long c0, int Q, long long N, const float *__restrict__ qb,
                                            const float *__restrict__ cbias, int head, const unsigned *__restrict__ mask, long long mask_w,
                                            unsigned long long *lists, unsigned long long *thr, int k) {
  const int i = threadIdx.x & 15;
  unsigned long long pend[4] = {0ull, 0ull, 0ull, 0ull};
  tile_epilogue(acc, q0, c0, Q, c0 + 64, qb, head,
                [&](int, int qrow) {
                  TopkRow st{0ull, {0u, 0u}, qrow - q0};
                  st.thr = lds_ld64(thr + st.lr);
                  if (mask) {
                    const long long w0 = c0 >> 5;
                    const unsigned *mrow = mask + (size_t)qrow * mask_w;
                    if (w0 < mask_w) st.w[0] = mrow[w0];                  // (the right half of a ragged last tile may start past N)
                    if (w0 + 1 < mask_w) st.w[1] = mrow[w0 + 1];
                  }
                  return st;
                },
                [&](long long col) { return cbias[col < N ? col : N - 1]; },
                [&](const TopkRow &st, int, int b, long long col, float sc_) {
                  const bool out = col >= N || ((st.w[b >> 1] >> (16 * (b & 1) + i)) & 1u) || sc_ == -INFINITY;
                  const unsigned long long key = topk_key(sc_, (unsigned)col);
                  pend[b] = (!out && key > st.thr) ? key : 0ull;
                  if (b == 3) topk_insert(pend, lists + (size_t)st.lr * k, thr + st.lr, k, st.thr);
                });
}

// dynamic LDS of the strip kernels: [4 waves][64 rows][k] keys, then [4][64] thresholds
__device__ __forceinline__ void topk_lds(unsigned long long *dyn, int k, unsigned long long *&lists, unsigned long long *&thr) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  lists = dyn + (size_t)wave * 64 * k;
  thr = dyn + (size_t)4 * 64 * k + wave * 64;
  for (int e = lane; e < 64 * k; e += 64) lds_st64(lists + e, 0ull);
  lds_st64(thr + lane, 0ull);
}

// a wave's lists -> partial[2 strip + candidate half of the wave][q][k]; empty slots go out as key 0
__device__ __forceinline__ void topk_store(const unsigned long long *lists, int q0, int Q, int k, unsigned long long *__restrict__ part) {
  const int lane = threadIdx.x & 63;
  const int n = min(64, Q - q0) * k;
  for (int e = lane; e < n; e += 64) part[(size_t)q0 * k + e] = lds_ld64(lists + e);
}

// Strip pass: the grid and ownership of rank_count_fused_kernel -- a workgroup owns one block of 128 queries and a strip of candidate
// tiles, a wave 64 rows x its 64-column half of every tile -- and the tile product of score_all_lds_kernel, so the scores are its bits.
template <bool VEC>
__global__ __launch_bounds__(WG) void topk_strip_kernel(
    const float *__restrict__ qvec, const float *__restrict__ qb, const float *__restrict__ nodes, const float *__restrict__ cbias,
    const unsigned *__restrict__ mask, long long mask_w, unsigned long long *__restrict__ partial,
    int Q, long long N, int d, int head, int q_blocks, int strips, int k) {
  __shared__ __attribute__((aligned(16))) float sA[2][128 * LDS_LD], sB[2][128 * LDS_LD];
  extern __shared__ __attribute__((aligned(16))) unsigned long long topk_dyn[];
  const int tid = threadIdx.x, wave = tid >> 6;
  const int qt = (blockIdx.x % q_blocks) * 128, strip = blockIdx.x / q_blocks;
  const long long n_tiles = (N + 127) / 128;
  const long long tile_end = strip_first(strip + 1, n_tiles, strips);
  const int sr = tid >> 2, q0 = qt + (wave >> 1) * 64;
  unsigned long long *lists, *thr;
  topk_lds(topk_dyn, k, lists, thr);
  const float *ga[2], *gb[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) ga[h] = qvec + (size_t)min(qt + sr + 64 * h, Q - 1) * d;
  for (long long tile = strip_first(strip, n_tiles, strips); tile < tile_end; ++tile) {
    const long long ct = tile * 128;
#pragma unroll
    for (int h = 0; h < 2; ++h) gb[h] = nodes + (size_t)min(ct + sr + 64 * h, N - 1) * d;
    f32x4 acc[4][4];
    tile_product_f32<VEC>(ga, gb, d, sA, sB, acc);
    int q0t = q0;                     // as in rank_count_fused_kernel: the rows' addresses are formed again for every tile
    asm volatile("" : "+v"(q0t));
    tile_select(acc, q0t, ct + (wave & 1) * 64, Q, N, qb, cbias, head, mask, mask_w, lists, thr, k);
  }
  if (q0 < Q) topk_store(lists, q0, Q, k, partial + (size_t)(2 * strip + (wave & 1)) * Q * k);
}

template <bool VEC>
__global__ __launch_bounds__(WG) void topk_strip_bf16_kernel(
    const uint16_t *__restrict__ qs, const float *__restrict__ qb, const uint16_t *__restrict__ nodes, const float *__restrict__ cbias,
    const unsigned *__restrict__ mask, long long mask_w, unsigned long long *__restrict__ partial,
    int Q, long long N, int d, int dpad, int head, int q_blocks, int strips, int k) {
  __shared__ __attribute__((aligned(16))) uint16_t sA[2][3][SLAB], sB[2][SLAB];
  extern __shared__ __attribute__((aligned(16))) unsigned long long topk_dyn[];
  const int tid = threadIdx.x, wave = tid >> 6;
  const int qt = (blockIdx.x % q_blocks) * 128, strip = blockIdx.x / q_blocks;
  const long long n_tiles = (N + 127) / 128;
  const long long tile_end = strip_first(strip + 1, n_tiles, strips);
  const int sr = tid >> 2, q0 = qt + (wave >> 1) * 64;
  unsigned long long *lists, *thr;
  topk_lds(topk_dyn, k, lists, thr);
  const uint16_t *ga[2], *gb[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) ga[h] = qs + (size_t)min(qt + sr + 64 * h, Q - 1) * dpad;
  for (long long tile = strip_first(strip, n_tiles, strips); tile < tile_end; ++tile) {
    const long long ct = tile * 128;
#pragma unroll
    for (int h = 0; h < 2; ++h) gb[h] = nodes + (size_t)min(ct + sr + 64 * h, N - 1) * d;
    f32x4 acc[4][4];
    tile_product_bf16<VEC>(ga, gb, (size_t)Q * dpad, d, dpad, sA, sB, acc);
    int q0t = q0;
    asm volatile("" : "+v"(q0t));
    tile_select(acc, q0t, ct + (wave & 1) * 64, Q, N, qb, cbias, head, mask, mask_w, lists, thr, k);
  }
  if (q0 < Q) topk_store(lists, q0, Q, k, partial + (size_t)(2 * strip + (wave & 1)) * Q * k);
}

// Merge pass, one wave per query: of the n_part lists of k keys the k largest, in k rounds -- round j takes the largest key below the
// one round j - 1 took (keys of a query are distinct).  Integers only: any order of the lists gives the same answer.  Key 0 = no
// candidate left: id -1, score -inf.
__global__ __launch_bounds__(WG) void topk_merge_kernel(const unsigned long long *__restrict__ partial, int n_part, int Q, int k,
                                                        long long *__restrict__ ids, float *__restrict__ scores) {
  const int q = blockIdx.x * (WG / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (q >= Q) return;
  const int m = n_part * k;
  unsigned long long prev = ~0ull;
  for (int j = 0; j < k; ++j) {
    unsigned long long best = 0ull;
    for (int e = lane; e < m; e += 64) {
      const int p = e / k;
      const unsigned long long v = partial[((size_t)p * Q + q) * k + (e - p * k)];
      best = (v < prev && v > best) ? v : best;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const unsigned long long o = __shfl_xor(best, off);
      best = o > best ? o : best;
    }
    if (lane == 0) {
      const unsigned hi = (unsigned)(best >> 32);
      const unsigned bits = (hi & 0x80000000u) ? (hi ^ 0x80000000u) : ~hi;
      ids[(size_t)q * k + j] = best ? (long long)(unsigned)~(unsigned)best : -1ll;
      scores[(size_t)q * k + j] = best ? __uint_as_float(bits) : -INFINITY;
    }
    prev = best;
  }
}

// filter bits: mask[fq][fn / 32] |= 1 << (fn % 32).  Integer OR: duplicates are harmless.  Ranking (keep_target = 0): an entry on a
// query's own target is dropped (a caller error in both routes; the materialised route would rank that query against -inf).  Prediction
// (keep_target != 0) has no target: every listed cell is set.
__global__ void rank_mask_kernel(unsigned *__restrict__ mask, long long mask_w, const int *__restrict__ fq, const int *__restrict__ fn,
                                 long long F, const long long *__restrict__ batch, int head, int keep_target) {
  for (long long e = (long long)blockIdx.x * WG + threadIdx.x; e < F; e += (long long)gridDim.x * WG) {
    const int q = fq[e], n = fn[e];
    if (keep_target || n != rank_target(batch, q, head)) atomicOr(mask + (size_t)q * mask_w + (n >> 5), 1u << (n & 31));
  }
}

// the strips' partials [n_part][Q] summed into the int64 outputs (integers: any order is exact)
__global__ __launch_bounds__(WG) void rank_reduce_kernel(const uint2 *__restrict__ partial, int n_part, int Q,
                                                         long long *__restrict__ greater, long long *__restrict__ ties) {
  const int q = blockIdx.x * WG + threadIdx.x;
  if (q >= Q) return;
  long long gs = 0, es = 0;
  for (int p = 0; p < n_part; ++p) {
    const uint2 v = partial[(size_t)p * Q + q];
    gs += v.x;
    es += v.y;
  }
  greater[q] = gs;
  ties[q] = es;
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

// ------------------------------------------------------------------ fused evaluator: entry points
namespace {

constexpr int64_t FUSED_CU_CAP = 512;          // the workspace of strips = 0 is sized for up to this many compute units
inline int64_t align16(int64_t b) { return (b + 15) / 16 * 16; }

// the library's choice of strips: two workgroups per compute unit (what the LDS slabs and the registers of the count kernels allow)
inline int64_t fused_default_strips(int64_t Q, int64_t n_nodes, int64_t n_cu) {
  const int64_t qbl = (Q + 127) / 128, n_tiles = (n_nodes + 127) / 128;
  return std::max<int64_t>(1, std::min(n_tiles, (2 * std::min(n_cu, FUSED_CU_CAP) + qbl - 1) / qbl));
}

struct FusedLayout { int64_t qv, qb, part, mask, total, mask_w; };

// strips = 0: room for the default of any device up to FUSED_CU_CAP units, by a bound that grows with Q and with N:
// strips * Q <= min(n_tiles * Q, 2 * CAP * 128 + Q)
inline FusedLayout fused_layout(int64_t Q, int64_t n_nodes, int32_t d, int64_t strips, bool bf16) {
  FusedLayout L;
  L.mask_w = (n_nodes + 31) / 32;
  const int64_t n_tiles = (n_nodes + 127) / 128;
  const int64_t cells = strips > 0 ? strips * Q : std::min(n_tiles * Q, 2 * FUSED_CU_CAP * 128 + Q);
  L.qv = 0;
  L.qb = L.qv + align16(bf16 ? 3 * Q * k_pad32(d) * (int64_t)sizeof(uint16_t) : Q * (int64_t)d * (int64_t)sizeof(float));
  L.part = L.qb + align16(2 * Q * (int64_t)sizeof(float));
  L.mask = L.part + align16(2 * cells * (int64_t)sizeof(uint2));
  L.total = L.mask + align16(Q * L.mask_w * (int64_t)sizeof(unsigned));
  return L;
}

template <bool BF16, class T>
int rank_fused(const char *name, const int64_t *batch, int64_t Q, int32_t head, const T *nodes, const float *rel, const float *sbias,
               const float *pbias, const float *obias, const int32_t *filt_q, const int32_t *filt_n, int64_t F, int32_t strips,
               void *workspace, int64_t *greater, int64_t *ties, float *tscore, int64_t n_nodes, int32_t d, void *stream) {
  if (Q < 0 || n_nodes <= 0 || d <= 0 || Q > INT32_MAX || F < 0 || strips < 0 || (F && (!filt_q || !filt_n)) ||
      (Q && (!batch || !nodes || !rel || !workspace || !greater || !ties || !tscore)) || (reinterpret_cast<uintptr_t>(workspace) & 15)) {
    rgcn_set_error("%s: bad argument (workspace: 16-byte aligned; strips >= 0; F > 0 needs both filter lists)", name);
    return RGCN_EINVAL;
  }
  if ((sbias != nullptr) != (pbias != nullptr) || (sbias != nullptr) != (obias != nullptr)) {
    rgcn_set_error("%s: biases must be all set or all NULL", name);
    return RGCN_EINVAL;
  }
  if (Q == 0) return RGCN_OK;
  int dev = 0, n_cu = 0;
  HIP_TRY(launch_device(&dev, &n_cu));
  const int64_t qbl = (Q + 127) / 128, n_tiles = (n_nodes + 127) / 128;
  const int64_t n_strips = strips > 0 ? strips : fused_default_strips(Q, n_nodes, n_cu);
  // a strip's counters are 32-bit: (tiles of the longest strip) * 128 cells per query
  if (n_strips * qbl > INT32_MAX || n_tiles > INT32_MAX || ((n_tiles + n_strips - 1) / n_strips + 1) * 128 > INT32_MAX) {
    rgcn_set_error("%s: too many scores in one call; split the batch", name);
    return RGCN_EUNSUPPORTED;
  }
  const FusedLayout L = fused_layout(Q, n_nodes, d, strips, BF16);
  char *ws = static_cast<char *>(workspace);
  float *qb = reinterpret_cast<float *>(ws + L.qb);
  uint2 *part = reinterpret_cast<uint2 *>(ws + L.part);
  unsigned *mask = F ? reinterpret_cast<unsigned *>(ws + L.mask) : nullptr;
  hipStream_t st = (hipStream_t)stream;
  const long long *b = reinterpret_cast<const long long *>(batch);
  const float *qb1 = sbias ? qb : nullptr, *cb1 = sbias ? (head ? sbias : obias) : nullptr;
  if (F) {
    HIP_TRY(zero_async(mask, (size_t)(Q * L.mask_w) * sizeof(unsigned), st));
    hipLaunchKernelGGL(rank_mask_kernel, dim3((unsigned)std::min<int64_t>((F + WG - 1) / WG, 1 << 16)), dim3(WG), 0, st, mask,
                       (long long)L.mask_w, filt_q, filt_n, (long long)F, b, head, 0);
  }
  const dim3 gq((unsigned)((Q + 3) / 4)), gt((unsigned)qbl), gc((unsigned)(n_strips * qbl));
  if constexpr (BF16) {
    uint16_t *qs = reinterpret_cast<uint16_t *>(ws + L.qv);
    const int dpad = (int)k_pad32(d);
    hipLaunchKernelGGL(rank_query_bf16_kernel, gq, dim3(WG), 0, st, b, (int)Q, head, nodes, rel, sbias, pbias, obias, qs, qb, d, dpad);
    // 16-byte loads of the entity rows as in rgcn_distmult_score_all_bf16: the same instantiation, the same bits
    auto run = [&](auto vec) {
      constexpr bool V = decltype(vec)::value;
      hipLaunchKernelGGL(rank_target_bf16_kernel<V>, gt, dim3(WG), 0, st, qs, qb1, nodes, cb1, b, tscore, (int)Q, d, dpad, head);
      hipLaunchKernelGGL(rank_count_fused_bf16_kernel<V>, gc, dim3(WG), 0, st, qs, qb1, nodes, cb1, tscore, mask, (long long)L.mask_w,
                         part, (int)Q, (long long)n_nodes, d, dpad, head, (int)qbl, (int)n_strips);
    };
    if (d % 8 == 0 && (reinterpret_cast<uintptr_t>(nodes) & 15) == 0) run(std::true_type{});
    else run(std::false_type{});
  } else {
    float *qvec = reinterpret_cast<float *>(ws + L.qv);
    hipLaunchKernelGGL(rank_query_kernel, gq, dim3(WG), 0, st, b, (int)Q, head, nodes, rel, sbias, pbias, obias, qvec, qb, d);
    auto run = [&](auto vec) {
      constexpr bool V = decltype(vec)::value;
      hipLaunchKernelGGL(rank_target_kernel<V>, gt, dim3(WG), 0, st, qvec, qb1, nodes, cb1, b, tscore, (int)Q, d, head);
      hipLaunchKernelGGL(rank_count_fused_kernel<V>, gc, dim3(WG), 0, st, qvec, qb1, nodes, cb1, tscore, mask, (long long)L.mask_w,
                         part, (int)Q, (long long)n_nodes, d, head, (int)qbl, (int)n_strips);
    };
    if (d % 4 == 0) run(std::true_type{});
    else run(std::false_type{});
  }
  hipLaunchKernelGGL(rank_reduce_kernel, dim3((unsigned)((Q + WG - 1) / WG)), dim3(WG), 0, st, part, (int)(2 * n_strips), (int)Q,
                     reinterpret_cast<long long *>(greater), reinterpret_cast<long long *>(ties));
  HIP_TRY(hipGetLastError());
  return RGCN_OK;
}

}  // namespace

extern "C" int64_t rgcn_distmult_rank_fused_workspace_bytes(int64_t Q, int64_t n_nodes, int32_t d, int32_t strips, int32_t bf16) {
  return (Q < 0 || n_nodes <= 0 || d <= 0 || strips < 0) ? 0 : fused_layout(Q, n_nodes, d, strips, bf16 != 0).total;
}

extern "C" int rgcn_distmult_rank_fused_f32(const int64_t *batch, int64_t Q, int32_t head, const float *nodes, const float *rel,
                                            const float *sbias, const float *pbias, const float *obias, const int32_t *filt_q,
                                            const int32_t *filt_n, int64_t F, int32_t strips, void *workspace, int64_t *greater,
                                            int64_t *ties, float *tscore, int64_t n_nodes, int32_t n_rel, int32_t d, void *stream) {
  (void)n_rel;
  return rank_fused<false>("distmult_rank_fused", batch, Q, head, nodes, rel, sbias, pbias, obias, filt_q, filt_n, F, strips, workspace,
                           greater, ties, tscore, n_nodes, d, stream);
}

extern "C" int rgcn_distmult_rank_fused_bf16(const int64_t *batch, int64_t Q, int32_t head, const uint16_t *nodes, const float *rel,
                                             const float *sbias, const float *pbias, const float *obias, const int32_t *filt_q,
                                             const int32_t *filt_n, int64_t F, int32_t strips, void *workspace, int64_t *greater,
                                             int64_t *ties, float *tscore, int64_t n_nodes, int32_t n_rel, int32_t d, void *stream) {
  (void)n_rel;
  return rank_fused<true>("distmult_rank_fused_bf16", batch, Q, head, nodes, rel, sbias, pbias, obias, filt_q, filt_n, F, strips, workspace,
                          greater, ties, tscore, n_nodes, d, stream);
}

// ------------------------------------------------------------------ top-k prediction: entry points
namespace {

constexpr int TOPK_LDS_CU = 160 * 1024;        // LDS of a compute unit: the static operand slabs and the lists share it

struct TopkLayout { int64_t qv, qb, part, mask, total, mask_w; };

// FusedLayout with k keys of 8 bytes per (strip half, query) in place of the (greater, equal) pair; the same `cells` bound
inline TopkLayout topk_layout(int64_t Q, int64_t n_nodes, int32_t d, int64_t k, int64_t strips, bool bf16) {
  TopkLayout L;
  L.mask_w = (n_nodes + 31) / 32;
  const int64_t n_tiles = (n_nodes + 127) / 128;
  const int64_t cells = strips > 0 ? strips * Q : std::min(n_tiles * Q, 2 * FUSED_CU_CAP * 128 + Q);
  L.qv = 0;
  L.qb = L.qv + align16(bf16 ? 3 * Q * k_pad32(d) * (int64_t)sizeof(uint16_t) : Q * (int64_t)d * (int64_t)sizeof(float));
  L.part = L.qb + align16(2 * Q * (int64_t)sizeof(float));
  L.mask = L.part + align16(2 * cells * k * (int64_t)sizeof(unsigned long long));
  L.total = L.mask + align16(Q * L.mask_w * (int64_t)sizeof(unsigned));
  return L;
}

template <bool BF16, class T>
int topk_fused(const char *name, const int64_t *batch, int64_t Q, int32_t head, const T *nodes, const float *rel, const float *sbias,
               const float *pbias, const float *obias, const int32_t *filt_q, const int32_t *filt_n, int64_t F, int32_t k, int32_t strips,
               void *workspace, int64_t *ids, float *scores, int64_t n_nodes, int32_t d, void *stream) {
  if (Q < 0 || n_nodes <= 0 || d <= 0 || Q > INT32_MAX || F < 0 || k < 1 || strips < 0 || (F && (!filt_q || !filt_n)) ||
      (Q && (!batch || !nodes || !rel || !workspace || !ids || !scores)) || (reinterpret_cast<uintptr_t>(workspace) & 15)) {
    rgcn_set_error("%s: bad argument (workspace: 16-byte aligned; k >= 1; strips >= 0; F > 0 needs both filter lists)", name);
    return RGCN_EINVAL;
  }
  if ((sbias != nullptr) != (pbias != nullptr) || (sbias != nullptr) != (obias != nullptr)) {
    rgcn_set_error("%s: biases must be all set or all NULL", name);
    return RGCN_EINVAL;
  }
  if (k > TOPK_MAX) {
    rgcn_set_error("%s: k = %d is above the native limit of %d; select from the materialised scores instead", name, (int)k, TOPK_MAX);
    return RGCN_EUNSUPPORTED;
  }
  if (n_nodes > INT32_MAX) {
    rgcn_set_error("%s: entity ids must fit 31 bits", name);
    return RGCN_EUNSUPPORTED;
  }
  if (Q == 0) return RGCN_OK;
  int dev = 0, n_cu = 0;
  HIP_TRY(launch_device(&dev, &n_cu));
  const int64_t qbl = (Q + 127) / 128;
  const int64_t n_strips = strips > 0 ? strips : fused_default_strips(Q, n_nodes, n_cu);
  if (n_strips * qbl > INT32_MAX || 2 * n_strips * k > INT32_MAX) {
    rgcn_set_error("%s: too many strips in one call; split the batch", name);
    return RGCN_EUNSUPPORTED;
  }
  const TopkLayout L = topk_layout(Q, n_nodes, d, k, strips, BF16);
  char *ws = static_cast<char *>(workspace);
  float *qb = reinterpret_cast<float *>(ws + L.qb);
  unsigned long long *part = reinterpret_cast<unsigned long long *>(ws + L.part);
  unsigned *mask = F ? reinterpret_cast<unsigned *>(ws + L.mask) : nullptr;
  hipStream_t st = (hipStream_t)stream;
  const long long *b = reinterpret_cast<const long long *>(batch);
  const float *qb1 = sbias ? qb : nullptr, *cb1 = sbias ? (head ? sbias : obias) : nullptr;
  if (F) {
    HIP_TRY(zero_async(mask, (size_t)(Q * L.mask_w) * sizeof(unsigned), st));
    hipLaunchKernelGGL(rank_mask_kernel, dim3((unsigned)std::min<int64_t>((F + WG - 1) / WG, 1 << 16)), dim3(WG), 0, st, mask,
                       (long long)L.mask_w, filt_q, filt_n, (long long)F, b, head, 1);
  }
  const dim3 gq((unsigned)((Q + 3) / 4)), gc((unsigned)(n_strips * qbl));
  const size_t lds = (size_t)4 * 64 * (k + 1) * sizeof(unsigned long long);       // the lists and thresholds, sized by this call's k
  // the slabs are static LDS: the lists may take what they leave of the compute unit
  constexpr size_t slabs = BF16 ? sizeof(uint16_t) * (2 * 3 * SLAB + 2 * SLAB) : sizeof(float) * (4 * 128 * LDS_LD);
  auto strip_pass = [&](auto kc, auto... args) -> hipError_t {
    constexpr auto kern = decltype(kc)::value;
    hipError_t e = allow_lds<kern>(dev, slabs + lds, (int)(TOPK_LDS_CU - slabs));
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, gc, dim3(WG), lds, st, args...);
    return hipSuccess;
  };
  if constexpr (BF16) {
    uint16_t *qs = reinterpret_cast<uint16_t *>(ws + L.qv);
    const int dpad = (int)k_pad32(d);
    hipLaunchKernelGGL(rank_query_bf16_kernel, gq, dim3(WG), 0, st, b, (int)Q, head, nodes, rel, sbias, pbias, obias, qs, qb, d, dpad);
    // 16-byte loads of the entity rows as in rgcn_distmult_score_all_bf16: the same instantiation, the same bits
    if (d % 8 == 0 && (reinterpret_cast<uintptr_t>(nodes) & 15) == 0)
      HIP_TRY(strip_pass(kern_c<topk_strip_bf16_kernel<true>>, (const uint16_t *)qs, qb1, nodes, cb1, (const unsigned *)mask,
                         (long long)L.mask_w, part, (int)Q, (long long)n_nodes, d, dpad, head, (int)qbl, (int)n_strips, (int)k));
    else
      HIP_TRY(strip_pass(kern_c<topk_strip_bf16_kernel<false>>, (const uint16_t *)qs, qb1, nodes, cb1, (const unsigned *)mask,
                         (long long)L.mask_w, part, (int)Q, (long long)n_nodes, d, dpad, head, (int)qbl, (int)n_strips, (int)k));
  } else {
    float *qvec = reinterpret_cast<float *>(ws + L.qv);
    hipLaunchKernelGGL(rank_query_kernel, gq, dim3(WG), 0, st, b, (int)Q, head, nodes, rel, sbias, pbias, obias, qvec, qb, d);
    if (d % 4 == 0)
      HIP_TRY(strip_pass(kern_c<topk_strip_kernel<true>>, (const float *)qvec, qb1, nodes, cb1, (const unsigned *)mask,
                         (long long)L.mask_w, part, (int)Q, (long long)n_nodes, d, head, (int)qbl, (int)n_strips, (int)k));
    else
      HIP_TRY(strip_pass(kern_c<topk_strip_kernel<false>>, (const float *)qvec, qb1, nodes, cb1, (const unsigned *)mask,
                         (long long)L.mask_w, part, (int)Q, (long long)n_nodes, d, head, (int)qbl, (int)n_strips, (int)k));
  }
  hipLaunchKernelGGL(topk_merge_kernel, gq, dim3(WG), 0, st, (const unsigned long long *)part, (int)(2 * n_strips), (int)Q, (int)k,
                     reinterpret_cast<long long *>(ids), scores);
  HIP_TRY(hipGetLastError());
  return RGCN_OK;
}

}  // namespace

extern "C" int64_t rgcn_distmult_topk_workspace_bytes(int64_t Q, int64_t n_nodes, int32_t d, int32_t k, int32_t strips, int32_t bf16) {
  return (Q < 0 || n_nodes <= 0 || d <= 0 || k < 1 || k > TOPK_MAX || strips < 0) ? 0 : topk_layout(Q, n_nodes, d, k, strips, bf16 != 0).total;
}

extern "C" int rgcn_distmult_topk_f32(const int64_t *batch, int64_t Q, int32_t head, const float *nodes, const float *rel,
                                      const float *sbias, const float *pbias, const float *obias, const int32_t *filt_q,
                                      const int32_t *filt_n, int64_t F, int32_t k, int32_t strips, void *workspace, int64_t *ids,
                                      float *scores, int64_t n_nodes, int32_t n_rel, int32_t d, void *stream) {
  (void)n_rel;
  return topk_fused<false>("distmult_topk", batch, Q, head, nodes, rel, sbias, pbias, obias, filt_q, filt_n, F, k, strips, workspace, ids,
                           scores, n_nodes, d, stream);
}

extern "C" int rgcn_distmult_topk_bf16(const int64_t *batch, int64_t Q, int32_t head, const uint16_t *nodes, const float *rel,
                                       const float *sbias, const float *pbias, const float *obias, const int32_t *filt_q,
                                       const int32_t *filt_n, int64_t F, int32_t k, int32_t strips, void *workspace, int64_t *ids,
                                       float *scores, int64_t n_nodes, int32_t n_rel, int32_t d, void *stream) {
  (void)n_rel;
  return topk_fused<true>("distmult_topk_bf16", batch, Q, head, nodes, rel, sbias, pbias, obias, filt_q, filt_n, F, k, strips, workspace, ids,
                          scores, n_nodes, d, stream);
}
