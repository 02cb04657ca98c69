// Ranking evaluator of the link-prediction experiments: every entity scored as the
// head or the tail of each test triple, known true triples masked, rank of the target counted with ties.
// Reference lines taken over: utils/misc.py:60-110 (evaluate: toscore expansion :78-83, model call :85,
// filter_scores :40-58, raw_ranks / num_ties :93-99) and torch_rgcn/layers.py:87-98 (DistMult.forward on the
// expanded [bn, N, 3] index tensor, which is what the reference scores -- three gathers of bn x N x d floats).
//
// Here the [bn, N, 3] index tensor is never built.  For a batch of Q queries
//     scores[q, n] = sum_k (nodes[fixed_q, k] * rel[p_q, k]) * nodes[n, k]  (+ biases)
// is an NT product of the Q x d query vectors with the N x d entity table: fp32 MFMA (v_mfma_f32_16x16x4_f32,
// exact fp32 products and accumulation): 128 x 128 scores per workgroup, operand slabs staged through double-buffered LDS
// (score_all_kernel).  The K index is permuted -- lane group kq carries k = 16t + 4kq + c at MFMA c of step t -- which is legal
// because both operands use the same permutation and the sum over k does not care.
// Second route (rgcn_distmult_rank_fused_*, utils/misc.py:40-58, 71-99): the same tile product with an epilogue that compares every score
// with the target's instead of storing it -- greater / ties per query without a [Q, N] buffer.  Third (rgcn_distmult_topk_*):
// an epilogue that selects the k best.  Fourth (rgcn_distmult_lse_*, rgcn_distmult_softmax_grad_*; an extension, the reference trains on
// sampled negatives only): an epilogue that adds exp(score) for the 1-N softmax loss, and the gradient cells of that loss in column chunks;
// with label smoothing (rgcn_distmult_lse_smooth_*, rgcn_distmult_softmax_grad_smooth_*) the epilogue also sums and counts the allowed scores.
// Fifth (rgcn_distmult_bce_sums_*, rgcn_distmult_bce_grad_*; an extension too): the K-vs-All binary cross-entropy -- the mask bits are
// LABELS, the epilogue sums softplus(score) over every cell and the scores of the positive ones, the gradient cells are sigmoid - label.
// Layout of the file: the two product loops (fp32, bf16) and the epilogues (store, count, select, add) first; then a tile-precision trait
// (TileF32 / TileBf16) and the kernel roles -- score_all_kernel, target_score_kernel, strip_count_kernel, strip_select_kernel,
// strip_lse_kernel, strip_lse_smooth_kernel, strip_bce_kernel, softmax_grad_kernel, bce_grad_kernel -- each written once over
// <Tile, VEC>; then the entry points: one per role and storage, each taking the filter (the labels of the BCE roles) as the lists
// (filt_q, filt_n, F) or as the device-resident index (fkeys, fptr, fvals, K) -- StripArgs carries both, strip_check refuses both at once.
#include <cmath>
#include <cstdlib>

#include "rgcn_device.h"      // HIP_TRY, f32x4, WG, the bf16 widen / round helpers

namespace {

// The query form code of the `head` argument (rgcn_hip.h): bit 0 is the direction -- which end of the triple is predicted, hence the
// candidate-side bias, the target column and the side of the filter lookup --, bit 1 the form of the query vector.  Only launch_query looks at
// the form, to choose the query kernel's instantiation; every kernel receives the direction.
__host__ __device__ __forceinline__ int query_dir(int head) { return head & RGCN_QUERY_HEAD; }

// One complex feature of a ComplEx query vector: a = the anchor row's (re, im), r = the relation's.  tail queries
// (s, p, ?): z = a r; head queries (?, p, o): z = conj(r) a -- in both the score of candidate n is qv . nodes[n] with qv = [Re z | Im z].
// Each element is two rounded products and one rounded add or subtract (contraction off), so a*b - c*d in fp32 on the host forms the same bits.
__device__ __forceinline__ void complex_query(int dir, float a_re, float a_im, float r_re, float r_im, float &re, float &im) {
#pragma clang fp contract(off)
  if (dir) {
    re = r_re * a_re + r_im * a_im;
    im = r_re * a_im - r_im * a_re;
  } else {
    re = a_re * r_re - a_im * r_im;
    im = a_re * r_im + a_im * r_re;
  }
}

// query vectors and the query-side bias terms; one wave per query.  CX: the ComplEx form, a lane owns complex feature k < d / 2 (a
// sibling instantiation chosen by launch_query: the DistMult one is the kernel it was).  head: the direction.
template <bool CX>
__global__ __launch_bounds__(WG) void rank_query_kernel(
    const long long *__restrict__ batch, int Q, int head, const float *__restrict__ nodes,
    const float *__restrict__ rel, const float *__restrict__ sbias, const float *__restrict__ pbias,
    const float *__restrict__ obias, float *__restrict__ qvec, float *__restrict__ qb, int d) {
  const int q = blockIdx.x * (WG / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (q >= Q) return;
  const long long s = batch[3 * q], p = batch[3 * q + 1], o = batch[3 * q + 2];
  const long long fixed = head ? o : s;
  if constexpr (CX) {
    const int h = d >> 1;
    const float *a = nodes + (size_t)fixed * d, *r = rel + (size_t)p * d;
    for (int k = lane; k < h; k += 64)
      complex_query(head, a[k], a[k + h], r[k], r[k + h], qvec[(size_t)q * d + k], qvec[(size_t)q * d + k + h]);
  } else {
    for (int k = lane; k < d; k += 64) qvec[(size_t)q * d + k] = nodes[(size_t)fixed * d + k] * rel[(size_t)p * d + k];
  }
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

// The product loop of one 128 x 128 tile, shared by the four kernel roles (TileF32::product): whoever instantiates it gets the same
// K permutation and the same MFMA chain per
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

// ------------------------------------------------------------------ fused evaluator: ranks without the score matrix
__device__ __forceinline__ long long rank_target(const long long *__restrict__ batch, int q, int head) { return batch[3 * q + (head ? 0 : 2)]; }

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

// ------------------------------------------------------------------ bf16 entity table
// The same product on v_mfma_f32_16x16x32_bf16.  The candidates are bf16 already; the query vector nodes[fixed] * rel[p] is an fp32
// number and is NOT rounded: it is written as three bf16 terms hi = rne(q), mid = rne(q - hi), lo = rne(q - hi - mid) whose sum is q
// exactly (24 significand bits = 3 x 8; the remainders are exact fp32 differences, formed with contraction off), and every bf16 x bf16 product is exact in fp32.  So the
// kernel adds the terms the fp32 evaluator adds on the widened table, in another order, at 3 of the 16x cheaper matrix instructions per
// 32 k instead of 8 fp32 ones per 32 k.
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// the fp32 query element v as three bf16 terms hi + mid + lo = v; the remainders are exact fp32 differences, formed with contraction off
__device__ __forceinline__ void query_terms(float v, uint16_t &hi, uint16_t &mid, uint16_t &lo) {
#pragma clang fp contract(off)
  hi = bf16_round(v);
  mid = lo = 0;
  if (v - v == 0.f) {                                    // finite (an inf / NaN element is its own hi: mid = lo = 0)
    if ((hi & 0x7FFFu) == 0x7F80u) hi = (hi & 0x8000u) | 0x7F7Fu;     // |v| above the largest bf16 rounds to inf: take the largest bf16, the
    const float r1 = v - bf16_widen(hi);                              // remainder (same binade: exact) goes to mid and lo
    mid = bf16_round(r1);
    lo = bf16_round(r1 - bf16_widen(mid));
  }
}

// query terms [3][Q][dpad] (dpad = d rounded up to the K step of 32, the tail zeroed here: the product kernel loads whole 16-byte
// pieces of these rows without a clamp or a mask) and the query-side bias terms; one wave per query.  CX: the ComplEx form -- the fp32
// element from the widened row and the fp32 relation (complex_query), split the same way.  head: the direction.
template <bool CX>
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
  auto put = [&](int k, uint16_t hi, uint16_t mid, uint16_t lo) {
    uint16_t *dst = qs + (size_t)q * dpad + k;
    dst[0] = hi;
    dst[term] = mid;
    dst[2 * term] = lo;
  };
  if constexpr (CX) {
    const int h = d >> 1;
    const uint16_t *a = nodes + (size_t)fixed * d;
    const float *r = rel + (size_t)p * d;
    for (int k = lane; k < h; k += 64) {
      float re, im;
      uint16_t hi, mid, lo;
      complex_query(head, bf16_widen(a[k]), bf16_widen(a[k + h]), r[k], r[k + h], re, im);
      query_terms(re, hi, mid, lo);
      put(k, hi, mid, lo);
      query_terms(im, hi, mid, lo);
      put(k + h, hi, mid, lo);
    }
    for (int k = d + lane; k < dpad; k += 64) put(k, 0, 0, 0);
  } else {
    for (int k = lane; k < dpad; k += 64) {
      uint16_t hi = 0, mid = 0, lo = 0;
      // the fp32 product as the fp32 evaluator forms it, then exact remainders: contraction is off in this function, a fused
      // fma(x, r, -hi) would split the unrounded product instead (closer to x r, but not what the fp32 kernel multiplies)
      if (k < d) query_terms(bf16_widen(nodes[(size_t)fixed * d + k]) * rel[(size_t)p * d + k], hi, mid, lo);
      put(k, hi, mid, lo);
    }
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

// The shape of the fp32 tile: 128 queries x 128 candidates per workgroup, 64 x 64 per wave, double-buffered LDS slabs, the loads
// of step t + 1 issued before the MFMAs of step t.  A K step is 32: a slab row is 32 bf16 = 64 bytes = four 16-byte pieces, lane
// 16 kq + i reads piece kq of row i (the operand map of v_mfma_f32_16x16x32_bf16: A[row l & 15][k = 8 (l >> 4) + j], B likewise by column)
// and uses each of its four B fragments against the hi, mid and lo A fragments: 48 MFMAs per step and wave behind 16 ds_read_b128.
// LDS rows are NOT padded: piece c of row r sits at piece c ^ ((r >> 2) & 2) of its 64 bytes.  A ds_read_b128 is served in four groups of
// 16 lanes that hold all 16 rows i, with piece a on rows 0-3 and 12-15 and piece a ^ 1 on rows 4-11; rows i, i + 4, i + 8, i + 12 share a
// 256-byte bank row, and with the swizzle they take pieces a, a ^ 1, a ^ 3, a ^ 2 of it: all distinct, no conflict.
constexpr int SLAB = 128 * 32;          // bf16 elements of one 128-row slab
__device__ __forceinline__ int slab_at(int row, int piece) { return row * 32 + 8 * (piece ^ ((row >> 2) & 2)); }

// The bf16 product loop of one tile, shared by the four kernel roles (TileBf16::product; as
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

// ------------------------------------------------------------------ 1-N softmax loss: log-sum-exp per query
// The product and epilogue once more, with an epilogue that ADDS: lse[q] = log sum exp(score) over the cells that are not filtered.
// Every row carries a pair (m, l): m = the largest score seen, l = sum exp(score - m) -- scores beyond +-88 occur, exp(score) alone
// overflows.  Two pairs merge as (max(m1, m2), l1 exp(m1 - m) + l2 exp(m2 - m)); the empty pair is (-inf, 0), and a merge against
// m = -inf subtracts 0 instead (-inf - -inf is NaN).  exp is __expf (v_exp_f32 on x log2 e): every argument is <= 0, a term's relative
// error is ~|x| 2^-23, and the terms with a large |x| are the ones that do not count.  exp(0) is exactly 1, so a row whose only cell is
// its target has l = 1.
__device__ __forceinline__ float row16_max_f(float v) {
  v = fmaxf(v, __int_as_float(dpp_i<0xB1>(__float_as_int(v), __float_as_int(v))));      // the four steps of tile_count
  v = fmaxf(v, __int_as_float(dpp_i<0x4E>(__float_as_int(v), __float_as_int(v))));
  v = fmaxf(v, __int_as_float(dpp_i<0x141>(__float_as_int(v), __float_as_int(v))));
  v = fmaxf(v, __int_as_float(dpp_i<0x140>(__float_as_int(v), __float_as_int(v))));
  return v;
}
__device__ __forceinline__ float row16_sum_f(float v) {       // a + b = b + a: after each exchange both partners hold the same bits
  v += __int_as_float(dpp_i<0xB1>(__float_as_int(v), __float_as_int(v)));
  v += __int_as_float(dpp_i<0x4E>(__float_as_int(v), __float_as_int(v)));
  v += __int_as_float(dpp_i<0x141>(__float_as_int(v), __float_as_int(v)));
  v += __int_as_float(dpp_i<0x140>(__float_as_int(v), __float_as_int(v)));
  return v;
}
__device__ __forceinline__ void lse_merge(float &m, float &l, float m2, float l2) {
  const float mn = fmaxf(m, m2), ref = mn == -INFINITY ? 0.f : mn;
  l = l * __expf(m - ref) + l2 * __expf(m2 - ref);
  m = mn;
}

// The adding epilogue of one tile: tile_epilogue over the wave's whole 64 x 64 block as tile_select runs it (n_cols = c0 + 64: the 16
// lanes of a row stay together; a column past N is clamped for its bias and counts as filtered), the mask words read as tile_count reads
// them.  A row's four cells per lane wait in p[]; at the fourth the row's maximum and then its sum go over the 16 lanes, and lane
// i = row keeps the tile's pair of that row -- merged into the wave's running (m, l) once per tile: two registers across the product.
// SMOOTH (label smoothing): beside the pair, the row's sum of the allowed scores -- the same cells as they go into p[], a masked cell
// or a column >= N adding 0 -- and the row's count of allowed cells: the clear bits of the row's two mask words among the columns of
// this half that exist, which every lane of the row holds already (no exchange).  Lane i = row keeps both over the tile's epilogue and
// then adds them, once per tile, into ITS OWN slot of the workgroup's LDS (t: the sums, c: the counts): no lane reads another's slot, so
// nothing synchronises, and no register more than the pair lives across the product.  m and l are formed by the same statements either
// way.
struct LseRow { unsigned w[2]; };

template <bool SMOOTH>
__device__ __forceinline__ void tile_lse(const f32x4 (&acc)[4][4], int q0, long long c0, int Q, long long N, const float *__restrict__ qb,
                                         const float *__restrict__ cbias, int head, const unsigned *__restrict__ mask, long long mask_w,
                                         float &m, float &l, float *__restrict__ t, int *__restrict__ c) {
  const int i = threadIdx.x & 15;
  float p[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
  float tm = -INFINITY, tl = 0.f, ts = 0.f, rs = 0.f;
  int tc = 0;
  const long long left = N - c0;                              // the columns of this half below N: bits [0, left) of the row's two words
  const unsigned long long valid = left >= 64 ? ~0ull : left <= 0 ? 0ull : (1ull << left) - 1;
  const unsigned valid0 = (unsigned)valid, valid1 = (unsigned)(valid >> 32);
  tile_epilogue(acc, q0, c0, Q, c0 + 64, qb, head,
                [&](int, int qrow) {
                  LseRow st{{0u, 0u}};
                  if (mask) {
                    const long long w0 = c0 >> 5;
                    const unsigned *mrow = mask + (size_t)qrow * mask_w;
                    if (w0 < mask_w) st.w[0] = mrow[w0];                  // (the right half of a ragged last tile may start past N)
                    if (w0 + 1 < mask_w) st.w[1] = mrow[w0 + 1];
                  }
                  return st;
                },
                [&](long long col) { return cbias[col < N ? col : N - 1]; },
                [&](const LseRow &st, int row, int b, long long col, float sc_) {
                  const bool out = col >= N || ((st.w[b >> 1] >> (16 * (b & 1) + i)) & 1u);
                  p[b] = out ? -INFINITY : sc_;
                  if constexpr (SMOOTH) rs = (b == 0 ? 0.f : rs) + (out ? 0.f : sc_);     // the decision p[] takes, 0 where p[] takes -inf
                  if (b == 3) {
                    const float rm = row16_max_f(fmaxf(fmaxf(p[0], p[1]), fmaxf(p[2], p[3])));
                    const float ref = rm == -INFINITY ? 0.f : rm;
                    const float rl = row16_sum_f((__expf(p[0] - ref) + __expf(p[1] - ref)) + (__expf(p[2] - ref) + __expf(p[3] - ref)));
                    tm = i == row ? rm : tm;
                    tl = i == row ? rl : tl;
                    if constexpr (SMOOTH) {
                      const float sum = row16_sum_f(rs);
                      ts = i == row ? sum : ts;
                      tc = i == row ? __popc(valid0 & ~st.w[0]) + __popc(valid1 & ~st.w[1]) : tc;
                    }
                  }
                });
  lse_merge(m, l, tm, tl);
  if constexpr (SMOOTH) { *t += ts; *c += tc; }               // (a row past Q: 0 + 0)
}

// a wave's pairs -> partial[2 strip + candidate half of the wave][q] = (m, l); the rows as strip_store maps them
__device__ __forceinline__ void lse_store(float m, float l, int q0, int Q, float2 *__restrict__ part) {
  const int lane = threadIdx.x & 63, i = lane & 15, kq = lane >> 4;
  const int qrow = q0 + 16 * (i >> 2) + 4 * kq + (i & 3);
  if (qrow < Q) part[qrow] = float2{m, l};
}
// the smoothed role's four: (m, l, t, the bits of the count c) -- one 16-byte store
__device__ __forceinline__ void lse_smooth_store(float m, float l, float t, int c, int q0, int Q, float4 *__restrict__ part) {
  const int lane = threadIdx.x & 63, i = lane & 15, kq = lane >> 4;
  const int qrow = q0 + 16 * (i >> 2) + 4 * kq + (i & 3);
  if (qrow < Q) part[qrow] = float4{m, l, t, __int_as_float(c)};
}

// ------------------------------------------------------------------ 1-N multi-label BCE loss: sums per query
// The K-vs-All binary cross-entropy: loss[q] = (1 / N) sum_n (softplus(s[q, n]) - y'[q, n] s[q, n]).  The mask bits are LABELS here -- a
// set bit is a positive cell (a known completion, or the query's own target: label_target_kernel) --, and no cell is left out: every
// column below N is in the sum, whatever its bit.  softplus(s) = max(s, 0) + log(1 + e) with e = exp(-|s|) in (0, 1]: nothing overflows
// for any finite score, and there is no running maximum to carry.  e is __expf (an argument <= 0, as in tile_lse).  The logarithm is
// taken once per FOUR cells (a lane's cells of one query row): sum log(1 + e_j) = log(1 + S) with S = prod (1 + e_j) - 1 <= 15, built
// as S <- S + e + S e, so that terms far below 1 keep their bits instead of vanishing in 1 + e.  log(1 + S) is __logf of a number in
// (1, 16], except below S = 2^-10, where 1 + S has lost S's low bits and the series S - S^2 / 2 (error S^3 / 3, 3e-7 of S there) is
// the better value.
__device__ __forceinline__ float bce_exp(float s) { return __expf(-fabsf(s)); }
__device__ __forceinline__ float bce_log1p(float S) { return S < 0x1p-10f ? S - 0.5f * S * S : __logf(1.f + S); }
// sigmoid(s) from the same e: 1 / (1 + e) for s >= 0, e / (1 + e) below -- no exp of a positive number
__device__ __forceinline__ float bce_sigmoid(float s) {
  const float e = bce_exp(s), r = __builtin_amdgcn_rcpf(1.f + e);
  return s >= 0.f ? r : e * r;
}

// The summing epilogue of one tile, run as tile_lse runs (n_cols = c0 + 64: the 16 lanes of a row stay together; a column past N is
// clamped for its bias and adds nothing).  Per query row three sums over the columns below N: sp += softplus(s) on every cell, ps += s
// on the cells whose label bit is set, and the count of those bits -- the set bits of the row's two mask words among the columns of this
// half that exist, which every lane of the row holds already.  A row's four cells per lane are added in the lane, then over the row's 16
// lanes, and lane i = row keeps the tile's sums: sp and ps go into the wave's two running registers once per tile (the two that
// strip_lse_kernel carries), the count into the lane's own LDS slot, as tile_lse<true> keeps its count.
__device__ __forceinline__ void tile_bce(const f32x4 (&acc)[4][4], int q0, long long c0, int Q, long long N, const float *__restrict__ qb,
                                         const float *__restrict__ cbias, int head, const unsigned *__restrict__ mask, long long mask_w,
                                         float &sp, float &ps, int *__restrict__ c) {
  const int i = threadIdx.x & 15;
  float tsp = 0.f, tps = 0.f, rsp = 0.f, rps = 0.f, rS = 0.f;
  int tc = 0;
  const long long left = N - c0;                              // the columns of this half below N: bits [0, left) of the row's two words
  const unsigned long long valid = left >= 64 ? ~0ull : left <= 0 ? 0ull : (1ull << left) - 1;
  const unsigned valid0 = (unsigned)valid, valid1 = (unsigned)(valid >> 32);
  tile_epilogue(acc, q0, c0, Q, c0 + 64, qb, head,
                [&](int, int qrow) {
                  LseRow st{{0u, 0u}};
                  const long long w0 = c0 >> 5;
                  const unsigned *mrow = mask + (size_t)qrow * mask_w;
                  if (w0 < mask_w) st.w[0] = mrow[w0];                    // (the right half of a ragged last tile may start past N)
                  if (w0 + 1 < mask_w) st.w[1] = mrow[w0 + 1];
                  return st;
                },
                [&](long long col) { return cbias[col < N ? col : N - 1]; },
                [&](const LseRow &st, int row, int b, long long col, float sc_) {
                  const bool in = col < N, pos = in && ((st.w[b >> 1] >> (16 * (b & 1) + i)) & 1u);
                  const float e = in ? bce_exp(sc_) : 0.f;                // (a column past N: the factor 1)
                  rS = b == 0 ? e : fmaf(rS, e, rS + e);
                  rsp = (b == 0 ? 0.f : rsp) + (in ? fmaxf(sc_, 0.f) : 0.f);
                  rps = (b == 0 ? 0.f : rps) + (pos ? sc_ : 0.f);
                  if (b == 3) {
                    const float s1 = row16_sum_f(rsp + bce_log1p(rS)), s2 = row16_sum_f(rps);
                    tsp = i == row ? s1 : tsp;
                    tps = i == row ? s2 : tps;
                    tc = i == row ? __popc(valid0 & st.w[0]) + __popc(valid1 & st.w[1]) : tc;
                  }
                });
  sp += tsp;
  ps += tps;
  *c += tc;                                                   // (a row past Q: 0)
}

// a wave's sums -> partial[2 strip + candidate half of the wave][q] = (sp, ps, the bits of the count, 0): one 16-byte store
__device__ __forceinline__ void bce_store(float sp, float ps, int c, int q0, int Q, float4 *__restrict__ part) {
  const int lane = threadIdx.x & 63, i = lane & 15, kq = lane >> 4;
  const int qrow = q0 + 16 * (i >> 2) + 4 * kq + (i & 3);
  if (qrow < Q) part[qrow] = float4{sp, ps, __int_as_float(c), 0.f};
}

// ------------------------------------------------------------------ the tile precision and the kernel roles
// What a kernel has to know about the storage of the entity table: the operand element type, the static LDS slabs of a workgroup, the
// stride of the query rows and which product loop runs.  Every role below is written once over <Tile, VEC> (VEC: 16-byte loads of the
// entity rows); the roles of one <Tile, VEC> share one product and tile_epilogue, hence the same bits for the same pair of rows.

// The operand facts of one call, the same shape for both storages.  The two operand pointers (q: the query rows, nodes: the entity table
// [N][d]) travel beside it as kernel parameters of their own: `__restrict__` does not hold on a struct member, and without it the strip
// kernels come out of the compiler differently (12 registers apart).
struct TileDims {
  int d, dpad;                // row length; d rounded up to the bf16 K step of 32 (fp32 does not read it)
  size_t term;                // bf16: Q * dpad, from a query row's hi term to its mid and from mid to lo (fp32 does not read it)
};

struct TileF32 {
  using elem = float;         // queries: fp32 [Q][d]
  struct Slabs { float a[2][128 * LDS_LD], b[2][128 * LDS_LD]; };             // 40,960 bytes
  static constexpr int strip_waves = 3;                                       // workgroups per CU = waves per SIMD that the slabs allow
  static __device__ __forceinline__ int q_stride(const TileDims &dm) { return dm.d; }
  template <bool VEC>
  static __device__ __forceinline__ void product(const float *const (&ga)[2], const float *const (&gb)[2], const TileDims &dm, Slabs &s,
                                                 f32x4 (&acc)[4][4]) {
    tile_product_f32<VEC>(ga, gb, dm.d, s.a, s.b, acc);
  }
};

struct TileBf16 {
  using elem = uint16_t;      // queries: the hi term of bf16 [3][Q][dpad]
  struct Slabs { uint16_t a[2][3][SLAB], b[2][SLAB]; };                       // 65,536 bytes
  static constexpr int strip_waves = 2;
  static __device__ __forceinline__ int q_stride(const TileDims &dm) { return dm.dpad; }
  template <bool VEC>
  static __device__ __forceinline__ void product(const uint16_t *const (&ga)[2], const uint16_t *const (&gb)[2], const TileDims &dm, Slabs &s,
                                                 f32x4 (&acc)[4][4]) {
    tile_product_bf16<VEC>(ga, gb, dm.term, dm.d, dm.dpad, s.a, s.b, acc);
  }
};

// this thread's two staging rows (tid >> 2 and + 64) of a slab that holds rows first .. first + 127 of `base`, clamped into its n rows
template <class E, class I>
__device__ __forceinline__ void stage_rows(const E *base, I first, I n, int ld, const E *(&g)[2]) {
  const int sr = threadIdx.x >> 2;
#pragma unroll
  for (int h = 0; h < 2; ++h) g[h] = base + (size_t)min(first + sr + 64 * h, n - 1) * ld;
}

// Score-all: one 128 x 128 tile per workgroup, every score stored.
template <class Tile, bool VEC>
__global__ __launch_bounds__(WG) void score_all_kernel(
    const typename Tile::elem *__restrict__ q, const typename Tile::elem *__restrict__ nodes, TileDims dm, const float *__restrict__ qb,
    const float *__restrict__ cbias, float *__restrict__ scores, int Q, long long N, int head, int q_blocks) {
  __shared__ __attribute__((aligned(16))) typename Tile::Slabs slabs;
  const int wave = threadIdx.x >> 6;
  const int qt = (blockIdx.x % q_blocks) * 128;
  const long long ct = (long long)(blockIdx.x / q_blocks) * 128;
  const typename Tile::elem *ga[2], *gb[2];
  stage_rows(q, qt, Q, Tile::q_stride(dm), ga);
  stage_rows(nodes, ct, N, dm.d, gb);
  f32x4 acc[4][4];
  Tile::template product<VEC>(ga, gb, dm, slabs, acc);
  tile_epilogue(acc, qt + (wave >> 1) * 64, ct + (wave & 1) * 64, Q, N, qb, head,
                [&](int, int qrow) { return scores + (size_t)qrow * N; },
                [&](long long col) { return cbias[col]; },
                [&](float *out, int, int, long long col, float sc_) { out[col] = sc_; });
}

// Target score (pass 2 of the fused evaluator): tscore[q] = the score of query q's own target, from the SAME product and epilogue as
// score-all -- one 128 x 128 tile per block of 128 queries whose "candidate" row j is nodes[target of query qt + j]; the diagonal cells
// are kept.
template <class Tile, bool VEC>
__global__ __launch_bounds__(WG) void target_score_kernel(
    const typename Tile::elem *__restrict__ q, const typename Tile::elem *__restrict__ nodes, TileDims dm, const float *__restrict__ qb,
    const float *__restrict__ cbias, const long long *__restrict__ batch, float *__restrict__ tscore, int Q, int head) {
  __shared__ __attribute__((aligned(16))) typename Tile::Slabs slabs;
  const int tid = threadIdx.x, wave = tid >> 6;
  const int qt = blockIdx.x * 128;
  const int sr = tid >> 2;
  const typename Tile::elem *ga[2], *gb[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int row = min(qt + sr + 64 * h, Q - 1);
    ga[h] = q + (size_t)row * Tile::q_stride(dm);
    gb[h] = nodes + (size_t)rank_target(batch, row, head) * dm.d;
  }
  f32x4 acc[4][4];
  Tile::template product<VEC>(ga, gb, dm, slabs, acc);
  tile_epilogue(acc, qt + (wave >> 1) * 64, (long long)qt + (wave & 1) * 64, Q, (long long)Q, qb, head,
                [&](int, int qrow) { return qrow; },
                [&](long long col) { return cbias[rank_target(batch, (int)col, head)]; },
                [&](int qrow, int, int, long long col, float sc_) { if (col == qrow) tscore[qrow] = sc_; });
}

// The strip walk of the count and the select kernel: a workgroup owns one block of 128 queries and a strip of candidate tiles, a wave
// 64 rows x its 64-column half of every tile; action(acc, q0, c0) takes the wave's finished 64 x 64 block.  What a wave keeps over its
// strip (counters, lists) is the caller's.  Returns where the wave stands: its first query row and its row of the partials.
struct StripWave { int q0, part; };

template <class Tile, bool VEC, class Action>
__device__ __forceinline__ StripWave strip_walk(const typename Tile::elem *q, const typename Tile::elem *nodes, const TileDims &dm,
                                                typename Tile::Slabs &slabs, int Q, long long N, int q_blocks, int strips, Action action) {
  const int wave = threadIdx.x >> 6;
  const int qt = (blockIdx.x % q_blocks) * 128, strip = blockIdx.x / q_blocks;
  const long long n_tiles = (N + 127) / 128;
  const long long tile_end = strip_first(strip + 1, n_tiles, strips);
  const int q0 = qt + (wave >> 1) * 64;
  const typename Tile::elem *ga[2], *gb[2];
  stage_rows(q, qt, Q, Tile::q_stride(dm), ga);
  for (long long tile = strip_first(strip, n_tiles, strips); tile < tile_end; ++tile) {
    const long long ct = tile * 128;
    stage_rows(nodes, ct, N, dm.d, gb);
    f32x4 acc[4][4];
    Tile::template product<VEC>(ga, gb, dm, slabs, acc);
    // the rows' target scores, thresholds, bias terms and addresses are formed again for every tile: hoisted out of this loop they would
    // sit in ~100 registers through the product, and the kernel would drop to one workgroup per compute unit
    int q0t = q0;
    asm volatile("" : "+v"(q0t));
    action(acc, q0t, ct + (wave & 1) * 64);
  }
  return {q0, 2 * strip + (wave & 1)};
}

// Strip count (pass 3 of the fused evaluator): counters stay in registers over the strip.
template <class Tile, bool VEC>
__global__ __launch_bounds__(WG) void strip_count_kernel(
    const typename Tile::elem *__restrict__ q, const typename Tile::elem *__restrict__ nodes, TileDims dm, const float *__restrict__ qb,
    const float *__restrict__ cbias, const float *__restrict__ tscore, const unsigned *__restrict__ mask, long long mask_w,
    uint2 *__restrict__ partial, int Q, long long N, int head, int q_blocks, int strips) {
  __shared__ __attribute__((aligned(16))) typename Tile::Slabs slabs;
  int g = 0, e = 0;
  const StripWave w = strip_walk<Tile, VEC>(q, nodes, dm, slabs, Q, N, q_blocks, strips, [&](const f32x4 (&acc)[4][4], int q0, long long c0) {
    tile_count(acc, q0, c0, Q, N, qb, cbias, head, tscore, mask, mask_w, g, e);
  });
  strip_store(g, e, w.q0, Q, partial + (size_t)w.part * Q);
}

// Strip select (top-k): the lists stay in LDS over the strip.
template <class Tile, bool VEC>
__global__ __launch_bounds__(WG) void strip_select_kernel(
    const typename Tile::elem *__restrict__ q, const typename Tile::elem *__restrict__ nodes, TileDims dm, const float *__restrict__ qb,
    const float *__restrict__ cbias, const unsigned *__restrict__ mask, long long mask_w, unsigned long long *__restrict__ partial,
    int Q, long long N, int head, int q_blocks, int strips, int k) {
  __shared__ __attribute__((aligned(16))) typename Tile::Slabs slabs;
  extern __shared__ __attribute__((aligned(16))) unsigned long long topk_dyn[];
  unsigned long long *lists, *thr;
  topk_lds(topk_dyn, k, lists, thr);
  const StripWave w = strip_walk<Tile, VEC>(q, nodes, dm, slabs, Q, N, q_blocks, strips, [&](const f32x4 (&acc)[4][4], int q0, long long c0) {
    tile_select(acc, q0, c0, Q, N, qb, cbias, head, mask, mask_w, lists, thr, k);
  });
  if (w.q0 < Q) topk_store(lists, w.q0, Q, k, partial + (size_t)w.part * Q * k);
}

// Strip log-sum-exp (1-N softmax loss): the wave's (m, l) pairs stay in registers over the strip; a strip without a tile writes (-inf, 0).
template <class Tile, bool VEC>
__global__ __launch_bounds__(WG) void strip_lse_kernel(
    const typename Tile::elem *__restrict__ q, const typename Tile::elem *__restrict__ nodes, TileDims dm, const float *__restrict__ qb,
    const float *__restrict__ cbias, const unsigned *__restrict__ mask, long long mask_w, float2 *__restrict__ partial, int Q, long long N,
    int head, int q_blocks, int strips) {
  __shared__ __attribute__((aligned(16))) typename Tile::Slabs slabs;
  float m = -INFINITY, l = 0.f;
  const StripWave w = strip_walk<Tile, VEC>(q, nodes, dm, slabs, Q, N, q_blocks, strips, [&](const f32x4 (&acc)[4][4], int q0, long long c0) {
    tile_lse<false>(acc, q0, c0, Q, N, qb, cbias, head, mask, mask_w, m, l, nullptr, nullptr);
  });
  lse_store(m, l, w.q0, Q, partial + (size_t)w.part * Q);
}

// The smoothed role of the strip pass (label smoothing): beside (m, l) the wave keeps t = the sum of the allowed scores and c = their
// count per query row -- in LDS, one slot per lane (2 KB beside the slabs: the workgroups per CU stay what the slabs allow), because
// two more registers across the product cost the fp32 element-load instantiation a workgroup per CU or a spill; the launch bound states
// the occupancy of strip_lse_kernel of the same <Tile, VEC>.  A strip without a tile writes (-inf, 0, 0, 0).
template <class Tile, bool VEC>
__global__ __launch_bounds__(WG, Tile::strip_waves) void strip_lse_smooth_kernel(
    const typename Tile::elem *__restrict__ q, const typename Tile::elem *__restrict__ nodes, TileDims dm, const float *__restrict__ qb,
    const float *__restrict__ cbias, const unsigned *__restrict__ mask, long long mask_w, float4 *__restrict__ partial, int Q, long long N,
    int head, int q_blocks, int strips) {
  __shared__ __attribute__((aligned(16))) typename Tile::Slabs slabs;
  __shared__ float t[WG];
  __shared__ int c[WG];
  t[threadIdx.x] = 0.f;
  c[threadIdx.x] = 0;
  float m = -INFINITY, l = 0.f;
  const StripWave w = strip_walk<Tile, VEC>(q, nodes, dm, slabs, Q, N, q_blocks, strips, [&](const f32x4 (&acc)[4][4], int q0, long long c0) {
    tile_lse<true>(acc, q0, c0, Q, N, qb, cbias, head, mask, mask_w, m, l, t + threadIdx.x, c + threadIdx.x);
  });
  lse_smooth_store(m, l, t[threadIdx.x], c[threadIdx.x], w.q0, Q, partial + (size_t)w.part * Q);
}

// the strips' pairs [n_part][Q] merged in index order (one answer for one `strips`); accurate expf / logf: Q values
__global__ __launch_bounds__(WG) void lse_merge_kernel(const float2 *__restrict__ partial, int n_part, int Q, float *__restrict__ lse) {
  const int q = blockIdx.x * WG + threadIdx.x;
  if (q >= Q) return;
  float m = -INFINITY, l = 0.f;
  for (int p = 0; p < n_part; ++p) {
    const float2 v = partial[(size_t)p * Q + q];
    const float mn = fmaxf(m, v.x);
    if (mn == -INFINITY) continue;                           // both empty: -inf - -inf would be NaN
    l = l * expf(m - mn) + v.y * expf(v.x - mn);
    m = mn;
  }
  lse[q] = m == -INFINITY ? -INFINITY : m + logf(l);
}

// the smoothed role's merge: (m, l) folded by the statements above -- the same lse bits --, t and c added in the same index order
__global__ __launch_bounds__(WG) void lse_smooth_merge_kernel(const float4 *__restrict__ partial, int n_part, int Q, float *__restrict__ lse,
                                                              float *__restrict__ ssum, int *__restrict__ cnt) {
  const int q = blockIdx.x * WG + threadIdx.x;
  if (q >= Q) return;
  float m = -INFINITY, l = 0.f, t = 0.f;
  int c = 0;
  for (int p = 0; p < n_part; ++p) {
    const float4 v = partial[(size_t)p * Q + q];
    t += v.z;
    c += __float_as_int(v.w);
    const float mn = fmaxf(m, v.x);
    if (mn == -INFINITY) continue;                           // both empty: -inf - -inf would be NaN
    l = l * expf(m - mn) + v.y * expf(v.x - mn);
    m = mn;
  }
  lse[q] = m == -INFINITY ? -INFINITY : m + logf(l);
  ssum[q] = t;
  cnt[q] = c;
}

// Strip sums (1-N BCE loss): sp and ps stay in registers over the strip -- the two that strip_lse_kernel carries --, the label count in
// LDS, one slot per lane, owned by that lane (1 KB beside the slabs; nothing synchronises).  The launch bound states the occupancy of
// strip_lse_kernel of the same <Tile, VEC>.  mask: the label bits, never NULL.  A strip without a tile writes zeros.
template <class Tile, bool VEC>
__global__ __launch_bounds__(WG, Tile::strip_waves) void strip_bce_kernel(
    const typename Tile::elem *__restrict__ q, const typename Tile::elem *__restrict__ nodes, TileDims dm, const float *__restrict__ qb,
    const float *__restrict__ cbias, const unsigned *__restrict__ mask, long long mask_w, float4 *__restrict__ partial, int Q, long long N,
    int head, int q_blocks, int strips) {
  __shared__ __attribute__((aligned(16))) typename Tile::Slabs slabs;
  __shared__ int c[WG];
  c[threadIdx.x] = 0;
  float sp = 0.f, ps = 0.f;
  const StripWave w = strip_walk<Tile, VEC>(q, nodes, dm, slabs, Q, N, q_blocks, strips, [&](const f32x4 (&acc)[4][4], int q0, long long c0) {
    tile_bce(acc, q0, c0, Q, N, qb, cbias, head, mask, mask_w, sp, ps, c + threadIdx.x);
  });
  bce_store(sp, ps, c[threadIdx.x], w.q0, Q, partial + (size_t)w.part * Q);
}

// the strips' sums [n_part][Q] added in index order (one answer for one `strips`)
__global__ __launch_bounds__(WG) void bce_merge_kernel(const float4 *__restrict__ partial, int n_part, int Q, float *__restrict__ sp,
                                                       float *__restrict__ ps, int *__restrict__ npos) {
  const int q = blockIdx.x * WG + threadIdx.x;
  if (q >= Q) return;
  float a = 0.f, b = 0.f;
  int c = 0;
  for (int p = 0; p < n_part; ++p) {
    const float4 v = partial[(size_t)p * Q + q];
    a += v.x;
    b += v.y;
    c += __float_as_int(v.z);
  }
  sp[q] = a;
  ps[q] = b;
  npos[q] = c;
}

// Gradient cells of the 1-N softmax loss, on the score-all grid cut to the candidate columns [c_first, c_first + c_count) (c_first a
// multiple of 128: tiles and mask words align as in tile_count): dS[q, c - c_first] = scale_q (exp(s[q, c] - lse[q]) - [c == target_q]),
// a filtered cell 0; scale_q = gscale[per_query ? q : 0] * inv_q -- the upstream gradient is read on the device.  mask: the filter
// bits of THIS chunk, [Q][mask_w] with bit 0 of word 0 = column c_first.  The product is recomputed by the product loop of the
// storage: s is bit for bit the cell the strip kernel of the same <Tile, VEC> added, so a row whose only cell is its target gets
// exp(0) - 1 = 0.  dS is fp32 for both storages.
// SMOOTH (label smoothing): dS = scale_q (exp(s - lse) - keep [c == target_q] - uni[q]) on an allowed cell, keep = keep[0] = 1 - eps and
// uni[q] = eps / (the allowed count of q) read on the device; without it keep is the constant 1 and nothing else is subtracted.
struct GradRow { float lse, scale, keep, uni; long long tgt; unsigned w[2]; float *out; };

template <class Tile, bool VEC, bool SMOOTH>
__global__ __launch_bounds__(WG) void softmax_grad_kernel(
    const typename Tile::elem *__restrict__ q, const typename Tile::elem *__restrict__ nodes, TileDims dm, const float *__restrict__ qb,
    const float *__restrict__ cbias, const long long *__restrict__ batch, const float *__restrict__ lse, const float *__restrict__ gscale,
    int per_query, float inv_q, const float *__restrict__ keep, const float *__restrict__ uni, const unsigned *__restrict__ mask,
    long long mask_w, float *__restrict__ dS, int Q, long long N, long long c_first, long long c_count, int head, int q_blocks) {
  __shared__ __attribute__((aligned(16))) typename Tile::Slabs slabs;
  const int wave = threadIdx.x >> 6, i = threadIdx.x & 15;
  const int qt = (blockIdx.x % q_blocks) * 128;
  const long long ct = c_first + (long long)(blockIdx.x / q_blocks) * 128;
  const typename Tile::elem *ga[2], *gb[2];
  stage_rows(q, qt, Q, Tile::q_stride(dm), ga);
  stage_rows(nodes, ct, N, dm.d, gb);
  f32x4 acc[4][4];
  Tile::template product<VEC>(ga, gb, dm, slabs, acc);
  const long long c0 = ct + (wave & 1) * 64;
  tile_epilogue(acc, qt + (wave >> 1) * 64, c0, Q, c_first + c_count, qb, head,
                [&](int, int qrow) {
                  GradRow st{lse[qrow], gscale[per_query ? qrow : 0] * inv_q, SMOOTH ? keep[0] : 1.f, SMOOTH ? uni[qrow] : 0.f,
                             rank_target(batch, qrow, head), {0u, 0u}, dS + (size_t)qrow * c_count - c_first};
                  if (mask) {
                    const long long w0 = (c0 - c_first) >> 5;
                    const unsigned *mrow = mask + (size_t)qrow * mask_w;
                    if (w0 < mask_w) st.w[0] = mrow[w0];
                    if (w0 + 1 < mask_w) st.w[1] = mrow[w0 + 1];
                  }
                  return st;
                },
                [&](long long col) { return cbias[col]; },
                [&](const GradRow &st, int, int b, long long col, float sc_) {
                  const bool out = (st.w[b >> 1] >> (16 * (b & 1) + i)) & 1u;
                  float p = __expf(sc_ - st.lse) - (col == st.tgt ? st.keep : 0.f);
                  if constexpr (SMOOTH) p -= st.uni;
                  st.out[col] = out ? 0.f : st.scale * p;
                });
}

// Gradient cells of the 1-N BCE loss, on the grid of softmax_grad_kernel over the candidate columns [c_first, c_first + c_count):
// dS[q, c - c_first] = scale_q (sigmoid(s[q, c]) - keep y[q, c] - uni), y the label bit of the cell in THIS chunk's mask (never NULL; the
// query's own target is among the bits), keep = 1 - eps and uni = eps / N plain arguments (1 and 0 without smoothing: one kernel).
// scale_q = gscale[per_query ? q : 0] * inv, read on the device.  EVERY cell of the chunk is written: a label is not a filter.  The
// product is the storage's product loop, so s is the cell strip_bce_kernel of the same <Tile, VEC> added.
struct BceRow { float scale; unsigned w[2]; float *out; };

template <class Tile, bool VEC>
__global__ __launch_bounds__(WG) void bce_grad_kernel(
    const typename Tile::elem *__restrict__ q, const typename Tile::elem *__restrict__ nodes, TileDims dm, const float *__restrict__ qb,
    const float *__restrict__ cbias, const float *__restrict__ gscale, int per_query, float inv, float keep, float uni,
    const unsigned *__restrict__ mask, long long mask_w, float *__restrict__ dS, int Q, long long N, long long c_first, long long c_count,
    int head, int q_blocks) {
  __shared__ __attribute__((aligned(16))) typename Tile::Slabs slabs;
  const int wave = threadIdx.x >> 6, i = threadIdx.x & 15;
  const int qt = (blockIdx.x % q_blocks) * 128;
  const long long ct = c_first + (long long)(blockIdx.x / q_blocks) * 128;
  const typename Tile::elem *ga[2], *gb[2];
  stage_rows(q, qt, Q, Tile::q_stride(dm), ga);
  stage_rows(nodes, ct, N, dm.d, gb);
  f32x4 acc[4][4];
  Tile::template product<VEC>(ga, gb, dm, slabs, acc);
  const long long c0 = ct + (wave & 1) * 64;
  tile_epilogue(acc, qt + (wave >> 1) * 64, c0, Q, c_first + c_count, qb, head,
                [&](int, int qrow) {
                  BceRow st{gscale[per_query ? qrow : 0] * inv, {0u, 0u}, dS + (size_t)qrow * c_count - c_first};
                  const long long w0 = (c0 - c_first) >> 5;
                  const unsigned *mrow = mask + (size_t)qrow * mask_w;
                  if (w0 < mask_w) st.w[0] = mrow[w0];
                  if (w0 + 1 < mask_w) st.w[1] = mrow[w0 + 1];
                  return st;
                },
                [&](long long col) { return cbias[col]; },
                [&](const BceRow &st, int, int b, long long col, float sc_) {
                  const bool pos = (st.w[b >> 1] >> (16 * (b & 1) + i)) & 1u;
                  st.out[col] = st.scale * ((bce_sigmoid(sc_) - (pos ? keep : 0.f)) - uni);
                });
}

// the filter bits of one chunk of candidate columns (rank_mask_kernel cut to [c_first, c_end); keep_target as there)
__global__ void chunk_mask_kernel(unsigned *__restrict__ mask, long long mask_w, const int *__restrict__ fq, const int *__restrict__ fn,
                                  long long F, const long long *__restrict__ batch, int head, int keep_target, long long c_first,
                                  long long c_end) {
  for (long long e = (long long)blockIdx.x * WG + threadIdx.x; e < F; e += (long long)gridDim.x * WG) {
    const int q = fq[e];
    const long long n = fn[e];
    if (n >= c_first && n < c_end && (keep_target || n != rank_target(batch, q, head)))
      atomicOr(mask + (size_t)q * mask_w + ((n - c_first) >> 5), 1u << ((n - c_first) & 31));
  }
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

// label bits (1-N BCE loss): a query's own target is a positive label whether it is listed or not -- one thread per query sets its bit
// in the mask of the columns [c_first, c_end), when the target lies inside them.  After this the mask IS the label matrix.
__global__ __launch_bounds__(WG) void label_target_kernel(unsigned *__restrict__ mask, long long mask_w, const long long *__restrict__ batch,
                                                          int Q, int head, long long c_first, long long c_end) {
  const int q = blockIdx.x * WG + threadIdx.x;
  if (q >= Q) return;
  const long long n = rank_target(batch, q, head);
  if (n >= c_first && n < c_end) atomicOr(mask + (size_t)q * mask_w + ((n - c_first) >> 5), 1u << ((n - c_first) & 31));
}

// ------------------------------------------------------------------ device-resident filter index
// The key -> completions table of one direction: keys [K] strictly ascending (key = p * N + the query's fixed entity), ptr [K + 1], vals
// ascending and unique within a key.  Validated once by its builder (functional.FilterIndex): nothing is range-checked here.
struct FilterIndexDev {
  const long long *keys, *ptr;
  const int *vals;
  long long K;
};

// first position in [lo, hi) whose element is not below x
template <class T>
__device__ __forceinline__ long long index_lower_bound(const T *__restrict__ a, long long lo, long long hi, long long x) {
  while (lo < hi) {
    const long long mid = lo + ((hi - lo) >> 1);
    if ((long long)a[mid] < x) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// The walk of one wave over the known completions of query q inside the columns [c_first, c_end): every lane forms the key and runs the
// same three searches (uniform over the wave), then the lanes stride the span by 64; f(n) takes a completion.  keep_target == 0 skips
// the query's own target.  A key that is absent has no completions.
template <class F>
__device__ __forceinline__ void index_walk(const FilterIndexDev &ix, const long long *__restrict__ batch, int q, int head, long long N,
                                           int keep_target, long long c_first, long long c_end, F f) {
  const int lane = threadIdx.x & 63;
  const long long key = batch[3 * q + 1] * N + batch[3 * q + (head ? 2 : 0)];
  const long long k = index_lower_bound(ix.keys, 0, ix.K, key);
  if (k >= ix.K || ix.keys[k] != key) return;
  const long long end = ix.ptr[k + 1];
  const long long lo = index_lower_bound(ix.vals, ix.ptr[k], end, c_first);
  const long long hi = index_lower_bound(ix.vals, lo, end, c_end);
  const long long tgt = rank_target(batch, q, head);
  for (long long e = lo + lane; e < hi; e += 64) {
    const long long n = ix.vals[e];
    if (keep_target || n != tgt) f(n);
  }
}

// filter bits from the index, one wave per query row: what rank_mask_kernel (c_first = 0, c_end = N) and chunk_mask_kernel set from the
// lists of the same completions; bit 0 of word 0 = column c_first
__global__ __launch_bounds__(WG) void index_mask_kernel(unsigned *__restrict__ mask, long long mask_w, FilterIndexDev ix,
                                                        const long long *__restrict__ batch, int Q, int head, long long N,
                                                        int keep_target, long long c_first, long long c_end) {
  const int q = blockIdx.x * (WG / 64) + (threadIdx.x >> 6);
  if (q >= Q) return;
  index_walk(ix, batch, q, head, N, keep_target, c_first, c_end, [&](long long n) {
    atomicOr(mask + (size_t)q * mask_w + ((n - c_first) >> 5), 1u << ((n - c_first) & 31));
  });
}

// the same walk for the materialised route: -inf where index_mask_kernel sets a bit of the whole row (ranking skips the target, as
// filter_scores does; prediction keeps it)
__global__ __launch_bounds__(WG) void index_filter_kernel(float *__restrict__ scores, FilterIndexDev ix, const long long *__restrict__ batch,
                                                          int Q, int head, long long N, int keep_target) {
  const int q = blockIdx.x * (WG / 64) + (threadIdx.x >> 6);
  if (q >= Q) return;
  index_walk(ix, batch, q, head, N, keep_target, 0, N, [&](long long n) { scores[(size_t)q * N + n] = -INFINITY; });
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

// ------------------------------------------------------------------ host side: what every entry point of a storage shares
template <class Tile>
constexpr bool is_bf16 = std::is_same<Tile, TileBf16>::value;

inline int64_t k_pad32(int32_t d) { return ((int64_t)d + 31) / 32 * 32; }

// The `head` argument of an entry point: one of the four query form codes, and an even width for the ComplEx forms (d = 0 where the
// entry builds no query vectors and ignores the form).  Sets the message and returns true on a bad one.
inline bool bad_query_form(const char *name, int32_t head, int32_t d) {
  if (head < 0 || head > (RGCN_QUERY_HEAD | RGCN_QUERY_COMPLEX)) {
    rgcn_set_error("%s: head = %d is no query form code (RGCN_QUERY_TAIL / RGCN_QUERY_HEAD, | RGCN_QUERY_COMPLEX)", name, (int)head);
    return true;
  }
  if ((head & RGCN_QUERY_COMPLEX) && (d & 1)) {
    rgcn_set_error("%s: the ComplEx query forms need an even width (real halves | imaginary halves), got d = %d", name, (int)d);
    return true;
  }
  return false;
}
inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

template <class Tile>
TileDims tile_dims(int64_t Q, int32_t d) {
  const int dpad = is_bf16<Tile> ? (int)k_pad32(d) : d;
  return {d, dpad, (size_t)Q * dpad};
}

// The load path of the entity rows, decided here for every role: f(true_type) launches the VEC instantiations, f(false_type) the element
// by element ones -- the same instantiation, the same bits on every route.  16-byte loads want fp32 rows of d % 4 == 0; bf16 rows of
// d % 8 == 0 on a 16-byte aligned table (WN18, FB15k-237).
template <class Tile, class F>
auto with_vec(const typename Tile::elem *nodes, int32_t d, F f) {
  const bool vec = is_bf16<Tile> ? d % 8 == 0 && aligned16(nodes) : d % 4 == 0;
  return vec ? f(std::true_type{}) : f(std::false_type{});
}

// the query kernel of the storage and of the form (head: the query form code; the kernels get the direction): q = fp32 query vectors
// [Q][d], or their three bf16 terms [3][Q][k_pad32(d)]
template <class Tile>
void launch_query(hipStream_t st, const long long *b, int64_t Q, int32_t head, const typename Tile::elem *nodes, const float *rel,
                  const float *sbias, const float *pbias, const float *obias, typename Tile::elem *q, float *qb, int32_t d) {
  const dim3 grid((unsigned)((Q + 3) / 4));
  const int dir = query_dir(head);
  auto go = [&](auto cx) {
    constexpr bool CX = decltype(cx)::value;
    if constexpr (is_bf16<Tile>)
      hipLaunchKernelGGL(rank_query_bf16_kernel<CX>, grid, dim3(WG), 0, st, b, (int)Q, dir, nodes, rel, sbias, pbias, obias, q, qb, d, (int)k_pad32(d));
    else
      hipLaunchKernelGGL(rank_query_kernel<CX>, grid, dim3(WG), 0, st, b, (int)Q, dir, nodes, rel, sbias, pbias, obias, q, qb, d);
  };
  if (head & RGCN_QUERY_COMPLEX) go(std::true_type{});
  else go(std::false_type{});
}

// q: the caller's scratch for launch_query; hint: what the storage adds to the argument message
template <class Tile>
int score_all(const char *name, const char *hint, const int64_t *batch, int64_t Q, int32_t head, const typename Tile::elem *nodes,
              const float *rel, const float *sbias, const float *pbias, const float *obias, typename Tile::elem *q, float *qbias,
              float *scores, int64_t n_nodes, int32_t d, void *stream) {
  if (Q < 0 || n_nodes <= 0 || d <= 0 || Q > INT32_MAX || (Q && (!batch || !nodes || !rel || !q || !scores)) ||
      (is_bf16<Tile> && !aligned16(q))) {
    rgcn_set_error("%s: bad argument%s", name, hint);
    return RGCN_EINVAL;
  }
  if ((sbias != nullptr) != (pbias != nullptr) || (sbias != nullptr) != (obias != nullptr) || (sbias && !qbias)) {
    rgcn_set_error("%s: biases must be all set (with the qbias scratch) or all NULL", name);
    return RGCN_EINVAL;
  }
  if (bad_query_form(name, head, d)) return RGCN_EINVAL;
  if (Q == 0) return RGCN_OK;
  const int dir = query_dir(head);
  const int qbl = (int)((Q + 127) / 128);
  const int64_t nwg = ((n_nodes + 127) / 128) * qbl;
  if (nwg > INT32_MAX) { rgcn_set_error("%s: too many scores in one call; split the batch", name); return RGCN_EUNSUPPORTED; }
  hipStream_t st = (hipStream_t)stream;
  launch_query<Tile>(st, reinterpret_cast<const long long *>(batch), Q, head, nodes, rel, sbias, pbias, obias, q, qbias, d);
  const float *qb1 = sbias ? qbias : nullptr, *cb1 = sbias ? (dir ? sbias : obias) : nullptr;
  with_vec<Tile>(nodes, d, [&](auto vec) {
    hipLaunchKernelGGL((score_all_kernel<Tile, decltype(vec)::value>), dim3((unsigned)nwg), dim3(WG), 0, st, (const typename Tile::elem *)q,
                       nodes, tile_dims<Tile>(Q, d), qb1, cb1, scores, (int)Q, (long long)n_nodes, dir, qbl);
  });
  HIP_TRY(hipGetLastError());
  return RGCN_OK;
}

}  // namespace

extern "C" int rgcn_distmult_score_all_f32(const int64_t *batch, int64_t Q, int32_t head, const float *nodes,
                                           const float *rel, const float *sbias, const float *pbias,
                                           const float *obias, float *qvec, float *qbias, float *scores,
                                           int64_t n_nodes, int32_t n_rel, int32_t d, void *stream) {
  (void)n_rel;
  return score_all<TileF32>("distmult_score_all", "", batch, Q, head, nodes, rel, sbias, pbias, obias, qvec, qbias, scores, n_nodes, d, stream);
}

extern "C" int64_t rgcn_distmult_score_all_bf16_workspace_bytes(int64_t Q, int32_t d) {
  return (Q < 0 || d <= 0) ? 0 : 3 * Q * k_pad32(d) * (int64_t)sizeof(uint16_t);
}

extern "C" int rgcn_distmult_score_all_bf16(const int64_t *batch, int64_t Q, int32_t head, const uint16_t *nodes,
                                            const float *rel, const float *sbias, const float *pbias,
                                            const float *obias, uint16_t *qsplit, float *qbias, float *scores,
                                            int64_t n_nodes, int32_t n_rel, int32_t d, void *stream) {
  (void)n_rel;
  return score_all<TileBf16>("distmult_score_all_bf16", " (qsplit: 16-byte aligned)", batch, Q, head, nodes, rel, sbias, pbias, obias, qsplit,
                             qbias, scores, n_nodes, d, stream);
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
  if (bad_query_form("rank_count", head, 0)) return RGCN_EINVAL;
  if (Q == 0) return RGCN_OK;
  hipLaunchKernelGGL(rank_count_kernel, dim3((unsigned)Q), dim3(WG), 0, (hipStream_t)stream, scores,
                     reinterpret_cast<const long long *>(batch), query_dir(head), (long long)n_nodes,
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

// The workspace of a query call: query vectors (fp32 [Q][d], or the three bf16 terms [3][Q][k_pad32(d)]) | query-side bias terms | the
// strips' partials | the filter bits of its n_cols candidate columns, [Q][ceil(n_cols / 32)].  bytes_per_cell: what a (strip half, query)
// cell of the partials holds -- the (greater, equal) pair of the evaluator, k keys of the top-k; 0 for the gradient cells, which have no
// strips and mask one chunk of columns.
// strips = 0: room for the default of any device up to FUSED_CU_CAP units, by a bound that grows with Q and with N:
// strips * Q <= min(n_tiles * Q, 2 * CAP * 128 + Q)
struct StripLayout { int64_t qv, qb, part, mask, total, mask_w; };

inline StripLayout strip_layout(int64_t Q, int64_t n_cols, int32_t d, int64_t strips, bool bf16, int64_t bytes_per_cell) {
  StripLayout L;
  L.mask_w = (n_cols + 31) / 32;
  const int64_t n_tiles = (n_cols + 127) / 128;
  const int64_t cells = strips > 0 ? strips * Q : std::min(n_tiles * Q, 2 * FUSED_CU_CAP * 128 + Q);
  L.qv = 0;
  L.qb = L.qv + align16(bf16 ? 3 * Q * k_pad32(d) * (int64_t)sizeof(uint16_t) : Q * (int64_t)d * (int64_t)sizeof(float));
  L.part = L.qb + align16(2 * Q * (int64_t)sizeof(float));
  L.mask = L.part + align16(2 * cells * bytes_per_cell);
  L.total = L.mask + align16(Q * L.mask_w * (int64_t)sizeof(unsigned));
  return L;
}

// what the strip entry points share of their C signatures, in that order
template <class E>
struct StripArgs {
  const char *name;
  const int64_t *batch;
  int64_t Q;
  int32_t head;                   // the query form code; the kernels past launch_query take dir()
  const E *nodes;
  const float *rel, *sbias, *pbias, *obias;
  const int32_t *filt_q, *filt_n;
  int64_t F;
  int32_t strips;
  void *workspace;
  int64_t n_nodes;
  int32_t d;
  void *stream;
  FilterIndexDev ix;              // the filter as an index: K > 0 fills the mask from it (then F = 0; strip_check refuses both)
  int32_t dir() const { return query_dir(head); }
};

inline FilterIndexDev filter_index(const int64_t *fkeys, const int64_t *fptr, const int32_t *fvals, int64_t K) {
  return {reinterpret_cast<const long long *>(fkeys), reinterpret_cast<const long long *>(fptr), fvals, (long long)K};
}
inline bool bad_index(const FilterIndexDev &ix) { return ix.K < 0 || (ix.K && (!ix.keys || !ix.ptr || !ix.vals)); }

// index_mask_kernel on a zeroed mask of the columns [c_first, c_end)
inline void launch_index_mask(hipStream_t st, unsigned *mask, int64_t mask_w, const FilterIndexDev &ix, const long long *b, int64_t Q,
                              int32_t head, int64_t n_nodes, int keep_target, int64_t c_first, int64_t c_end) {
  hipLaunchKernelGGL(index_mask_kernel, dim3((unsigned)((Q + WG / 64 - 1) / (WG / 64))), dim3(WG), 0, st, mask, (long long)mask_w, ix, b, (int)Q,
                     head, (long long)n_nodes, keep_target, (long long)c_first, (long long)c_end);
}

// Argument and bias checks of a strip entry point.  bad_own: the caller's conditions on its own arguments; hint: what they add to the message.
template <class E>
int strip_check(const StripArgs<E> &a, bool bad_own, const char *hint) {
  if (a.Q < 0 || a.n_nodes <= 0 || a.d <= 0 || a.Q > INT32_MAX || a.F < 0 || a.strips < 0 || bad_own || (a.F && (!a.filt_q || !a.filt_n)) ||
      (a.Q && (!a.batch || !a.nodes || !a.rel || !a.workspace)) || !aligned16(a.workspace)) {
    rgcn_set_error("%s: bad argument (workspace: 16-byte aligned; %sstrips >= 0; F > 0 needs both filter lists)", a.name, hint);
    return RGCN_EINVAL;
  }
  if (bad_index(a.ix) || (a.ix.K && a.F)) {
    rgcn_set_error("%s: bad filter index (K >= 0; K > 0 needs keys, ptr and vals, and no filter lists beside them)", a.name);
    return RGCN_EINVAL;
  }
  if ((a.sbias != nullptr) != (a.pbias != nullptr) || (a.sbias != nullptr) != (a.obias != nullptr)) {
    rgcn_set_error("%s: biases must be all set or all NULL", a.name);
    return RGCN_EINVAL;
  }
  if (bad_query_form(a.name, a.head, a.d)) return RGCN_EINVAL;
  return RGCN_OK;
}

// a query call that passed its checks (Q > 0): the grid, the carved workspace and the operands of its kernels
template <class Tile>
struct StripCall {
  int dev;                        // dev, n_strips, part: the strip roles only
  int64_t qbl, n_strips, mask_w;
  hipStream_t st;
  const long long *b;
  const typename Tile::elem *q;
  TileDims dm;
  const float *qb, *cbias;        // NULL without biases
  void *part;
  const unsigned *mask;           // NULL without a filter
};

// What every role does before its own kernels: the workspace carved (strip_layout over the columns [c_first, c_first + c_count)), the
// operand fields of `c` filled, the filter bits of those columns built and the query kernel of the storage launched.  chunk: the mask is
// a chunk's (the gradient cells) and chunk_mask_kernel fills it from the lists; else it spans the table and rank_mask_kernel does.
// labels (the 1-N BCE loss): the bits are labels, not a filter -- the mask exists whatever the lists or the index hold, and
// label_target_kernel sets every query's own target in it.
template <class Tile>
int query_begin(const StripArgs<typename Tile::elem> &a, int64_t bytes_per_cell, int keep_target, bool chunk, int64_t c_first, int64_t c_count,
                StripCall<Tile> &c, bool labels = false) {
  const StripLayout L = strip_layout(a.Q, c_count, a.d, a.strips, is_bf16<Tile>, bytes_per_cell);
  char *ws = static_cast<char *>(a.workspace);
  typename Tile::elem *q = reinterpret_cast<typename Tile::elem *>(ws + L.qv);
  float *qb = reinterpret_cast<float *>(ws + L.qb);
  unsigned *mask = (a.F || a.ix.K || labels) ? reinterpret_cast<unsigned *>(ws + L.mask) : nullptr;
  c.qbl = (a.Q + 127) / 128;
  c.mask_w = L.mask_w;
  c.st = (hipStream_t)a.stream;
  c.b = reinterpret_cast<const long long *>(a.batch);
  c.q = q;
  c.dm = tile_dims<Tile>(a.Q, a.d);
  c.qb = a.sbias ? qb : nullptr;
  c.cbias = a.sbias ? (a.dir() ? a.sbias : a.obias) : nullptr;
  c.part = ws + L.part;
  c.mask = mask;
  if (mask) HIP_TRY(zero_async(mask, (size_t)(a.Q * L.mask_w) * sizeof(unsigned), c.st));
  const dim3 list_grid((unsigned)std::min<int64_t>((a.F + WG - 1) / WG, 1 << 16));
  if (a.F && chunk)
    hipLaunchKernelGGL(chunk_mask_kernel, list_grid, dim3(WG), 0, c.st, mask, (long long)L.mask_w, a.filt_q, a.filt_n, (long long)a.F, c.b, a.dir(),
                       keep_target, (long long)c_first, (long long)(c_first + c_count));
  else if (a.F)
    hipLaunchKernelGGL(rank_mask_kernel, list_grid, dim3(WG), 0, c.st, mask, (long long)L.mask_w, a.filt_q, a.filt_n, (long long)a.F, c.b, a.dir(),
                       keep_target);
  if (a.ix.K) launch_index_mask(c.st, mask, L.mask_w, a.ix, c.b, a.Q, a.dir(), a.n_nodes, keep_target, c_first, c_first + c_count);
  if (labels)
    hipLaunchKernelGGL(label_target_kernel, dim3((unsigned)((a.Q + WG - 1) / WG)), dim3(WG), 0, c.st, mask, (long long)L.mask_w, c.b, (int)a.Q,
                       a.dir(), (long long)c_first, (long long)(c_first + c_count));
  launch_query<Tile>(c.st, c.b, a.Q, a.head, a.nodes, a.rel, a.sbias, a.pbias, a.obias, q, qb, a.d);
  return RGCN_OK;
}

// The preamble of a strip role: the strips (too_many(n_strips): the caller's bound on them, `what` names it in the message), then
// query_begin over the whole table.
template <class Tile, class TooMany>
int strip_begin(const StripArgs<typename Tile::elem> &a, int64_t bytes_per_cell, int keep_target, TooMany too_many, const char *what,
                StripCall<Tile> &c, bool labels = false) {
  int n_cu = 0;
  HIP_TRY(launch_device(&c.dev, &n_cu));
  const int64_t qbl = (a.Q + 127) / 128;
  c.n_strips = a.strips > 0 ? a.strips : fused_default_strips(a.Q, a.n_nodes, n_cu);
  if (c.n_strips * qbl > INT32_MAX || too_many(c.n_strips)) {
    rgcn_set_error("%s: too many %s in one call; split the batch", a.name, what);
    return RGCN_EUNSUPPORTED;
  }
  return query_begin<Tile>(a, bytes_per_cell, keep_target, false, 0, a.n_nodes, c, labels);
}

template <class Tile>
int rank_fused(const StripArgs<typename Tile::elem> &a, int64_t *greater, int64_t *ties, float *tscore) {
  if (int rc = strip_check(a, a.Q && (!greater || !ties || !tscore), "")) return rc;
  if (a.Q == 0) return RGCN_OK;
  StripCall<Tile> c;
  const int64_t n_tiles = (a.n_nodes + 127) / 128;
  // a strip's counters are 32-bit: (tiles of the longest strip) * 128 cells per query
  auto too_many = [&](int64_t n_strips) { return n_tiles > INT32_MAX || ((n_tiles + n_strips - 1) / n_strips + 1) * 128 > INT32_MAX; };
  if (int rc = strip_begin<Tile>(a, sizeof(uint2), 0, too_many, "scores", c)) return rc;
  uint2 *part = static_cast<uint2 *>(c.part);
  const int Q = (int)a.Q;
  with_vec<Tile>(a.nodes, a.d, [&](auto vec) {
    constexpr bool V = decltype(vec)::value;
    hipLaunchKernelGGL((target_score_kernel<Tile, V>), dim3((unsigned)c.qbl), dim3(WG), 0, c.st, c.q, a.nodes, c.dm, c.qb, c.cbias, c.b, tscore, Q,
                       a.dir());
    hipLaunchKernelGGL((strip_count_kernel<Tile, V>), dim3((unsigned)(c.n_strips * c.qbl)), dim3(WG), 0, c.st, c.q, a.nodes, c.dm, c.qb, c.cbias,
                       (const float *)tscore, c.mask, (long long)c.mask_w, part, Q, (long long)a.n_nodes, a.dir(), (int)c.qbl, (int)c.n_strips);
  });
  hipLaunchKernelGGL(rank_reduce_kernel, dim3((unsigned)((a.Q + WG - 1) / WG)), dim3(WG), 0, c.st, (const uint2 *)part, (int)(2 * c.n_strips), Q,
                     reinterpret_cast<long long *>(greater), reinterpret_cast<long long *>(ties));
  HIP_TRY(hipGetLastError());
  return RGCN_OK;
}

}  // namespace

extern "C" int64_t rgcn_distmult_rank_fused_workspace_bytes(int64_t Q, int64_t n_nodes, int32_t d, int32_t strips, int32_t bf16) {
  return (Q < 0 || n_nodes <= 0 || d <= 0 || strips < 0) ? 0 : strip_layout(Q, n_nodes, d, strips, bf16 != 0, sizeof(uint2)).total;
}

extern "C" int rgcn_distmult_rank_fused_f32(const int64_t *batch, int64_t Q, int32_t head, const float *nodes, const float *rel,
                                            const float *sbias, const float *pbias, const float *obias, const int32_t *filt_q,
                                            const int32_t *filt_n, int64_t F, const int64_t *fkeys, const int64_t *fptr,
                                            const int32_t *fvals, int64_t K, int32_t strips, void *workspace, int64_t *greater,
                                            int64_t *ties, float *tscore, int64_t n_nodes, int32_t n_rel, int32_t d, void *stream) {
  (void)n_rel;
  return rank_fused<TileF32>({"distmult_rank_fused", batch, Q, head, nodes, rel, sbias, pbias, obias, filt_q, filt_n, F, strips, workspace,
                              n_nodes, d, stream, filter_index(fkeys, fptr, fvals, K)}, greater, ties, tscore);
}

extern "C" int rgcn_distmult_rank_fused_bf16(const int64_t *batch, int64_t Q, int32_t head, const uint16_t *nodes, const float *rel,
                                             const float *sbias, const float *pbias, const float *obias, const int32_t *filt_q,
                                             const int32_t *filt_n, int64_t F, const int64_t *fkeys, const int64_t *fptr,
                                             const int32_t *fvals, int64_t K, int32_t strips, void *workspace, int64_t *greater,
                                             int64_t *ties, float *tscore, int64_t n_nodes, int32_t n_rel, int32_t d, void *stream) {
  (void)n_rel;
  return rank_fused<TileBf16>({"distmult_rank_fused_bf16", batch, Q, head, nodes, rel, sbias, pbias, obias, filt_q, filt_n, F, strips,
                               workspace, n_nodes, d, stream, filter_index(fkeys, fptr, fvals, K)}, greater, ties, tscore);
}

// ------------------------------------------------------------------ top-k prediction: entry points
namespace {

constexpr int TOPK_LDS_CU = 160 * 1024;        // LDS of a compute unit: the static operand slabs and the lists share it

inline int64_t topk_cell_bytes(int64_t k) { return k * (int64_t)sizeof(unsigned long long); }       // k keys per (strip half, query)

template <class Tile>
int topk_fused(const StripArgs<typename Tile::elem> &a, int32_t k, int64_t *ids, float *scores) {
  if (int rc = strip_check(a, k < 1 || (a.Q && (!ids || !scores)), "k >= 1; ")) return rc;
  if (k > TOPK_MAX) {
    rgcn_set_error("%s: k = %d is above the native limit of %d; select from the materialised scores instead", a.name, (int)k, TOPK_MAX);
    return RGCN_EUNSUPPORTED;
  }
  if (a.n_nodes > INT32_MAX) {
    rgcn_set_error("%s: entity ids must fit 31 bits", a.name);
    return RGCN_EUNSUPPORTED;
  }
  if (a.Q == 0) return RGCN_OK;
  StripCall<Tile> c;
  auto too_many = [&](int64_t n_strips) { return 2 * n_strips * k > INT32_MAX; };
  if (int rc = strip_begin<Tile>(a, topk_cell_bytes(k), 1, too_many, "strips", c)) return rc;
  unsigned long long *part = static_cast<unsigned long long *>(c.part);
  const size_t lds = (size_t)4 * 64 * (k + 1) * sizeof(unsigned long long);       // the lists and thresholds, sized by this call's k
  // the slabs are static LDS: the lists may take what they leave of the compute unit
  constexpr size_t slabs = sizeof(typename Tile::Slabs);
  HIP_TRY(with_vec<Tile>(a.nodes, a.d, [&](auto vec) -> hipError_t {
    constexpr auto kern = strip_select_kernel<Tile, decltype(vec)::value>;
    hipError_t e = allow_lds<kern>(c.dev, slabs + lds, (int)(TOPK_LDS_CU - slabs));
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, dim3((unsigned)(c.n_strips * c.qbl)), dim3(WG), lds, c.st, c.q, a.nodes, c.dm, c.qb, c.cbias, c.mask, (long long)c.mask_w, part,
                       (int)a.Q, (long long)a.n_nodes, a.dir(), (int)c.qbl, (int)c.n_strips, (int)k);
    return hipSuccess;
  }));
  hipLaunchKernelGGL(topk_merge_kernel, dim3((unsigned)((a.Q + 3) / 4)), dim3(WG), 0, c.st, (const unsigned long long *)part,
                     (int)(2 * c.n_strips), (int)a.Q, (int)k, reinterpret_cast<long long *>(ids), scores);
  HIP_TRY(hipGetLastError());
  return RGCN_OK;
}

}  // namespace

extern "C" int64_t rgcn_distmult_topk_workspace_bytes(int64_t Q, int64_t n_nodes, int32_t d, int32_t k, int32_t strips, int32_t bf16) {
  return (Q < 0 || n_nodes <= 0 || d <= 0 || k < 1 || k > TOPK_MAX || strips < 0)
             ? 0 : strip_layout(Q, n_nodes, d, strips, bf16 != 0, topk_cell_bytes(k)).total;
}

extern "C" int rgcn_distmult_topk_f32(const int64_t *batch, int64_t Q, int32_t head, const float *nodes, const float *rel,
                                      const float *sbias, const float *pbias, const float *obias, const int32_t *filt_q,
                                      const int32_t *filt_n, int64_t F, const int64_t *fkeys, const int64_t *fptr, const int32_t *fvals,
                                      int64_t K, int32_t k, int32_t strips, void *workspace, int64_t *ids, float *scores, int64_t n_nodes,
                                      int32_t n_rel, int32_t d, void *stream) {
  (void)n_rel;
  return topk_fused<TileF32>({"distmult_topk", batch, Q, head, nodes, rel, sbias, pbias, obias, filt_q, filt_n, F, strips, workspace,
                              n_nodes, d, stream, filter_index(fkeys, fptr, fvals, K)}, k, ids, scores);
}

extern "C" int rgcn_distmult_topk_bf16(const int64_t *batch, int64_t Q, int32_t head, const uint16_t *nodes, const float *rel,
                                       const float *sbias, const float *pbias, const float *obias, const int32_t *filt_q,
                                       const int32_t *filt_n, int64_t F, const int64_t *fkeys, const int64_t *fptr, const int32_t *fvals,
                                       int64_t K, int32_t k, int32_t strips, void *workspace, int64_t *ids, float *scores, int64_t n_nodes,
                                       int32_t n_rel, int32_t d, void *stream) {
  (void)n_rel;
  return topk_fused<TileBf16>({"distmult_topk_bf16", batch, Q, head, nodes, rel, sbias, pbias, obias, filt_q, filt_n, F, strips, workspace,
                               n_nodes, d, stream, filter_index(fkeys, fptr, fvals, K)}, k, ids, scores);
}

// ------------------------------------------------------------------ 1-N softmax loss: entry points
namespace {

// smooth: the smoothed role -- ssum [Q] and cnt [Q] beside lse and tscore, four floats per cell of the partials
template <class Tile>
int lse_fused(const StripArgs<typename Tile::elem> &a, float *lse, float *tscore, bool smooth = false, float *ssum = nullptr,
              int32_t *cnt = nullptr) {
  if (int rc = strip_check(a, a.Q && (!lse || !tscore || (smooth && (!ssum || !cnt))), "")) return rc;
  if (a.Q == 0) return RGCN_OK;
  StripCall<Tile> c;
  // the pairs are floats: no counter to overflow; the smoothed role counts a query's allowed entities in 32 bits
  auto too_many = [&](int64_t) { return smooth && a.n_nodes > INT32_MAX; };
  if (int rc = strip_begin<Tile>(a, smooth ? sizeof(float4) : sizeof(float2), 0, too_many, smooth ? "entities" : "strips", c)) return rc;
  const int Q = (int)a.Q;
  const dim3 strip_grid((unsigned)(c.n_strips * c.qbl)), merge_grid((unsigned)((a.Q + WG - 1) / WG));
  with_vec<Tile>(a.nodes, a.d, [&](auto vec) {
    hipLaunchKernelGGL((target_score_kernel<Tile, decltype(vec)::value>), dim3((unsigned)c.qbl), dim3(WG), 0, c.st, c.q, a.nodes, c.dm, c.qb, c.cbias,
                       c.b, tscore, Q, a.dir());
  });
  auto strip = [&](auto kern, auto *part) {
    hipLaunchKernelGGL(kern, strip_grid, dim3(WG), 0, c.st, c.q, a.nodes, c.dm, c.qb, c.cbias, c.mask, (long long)c.mask_w, part, Q,
                       (long long)a.n_nodes, a.dir(), (int)c.qbl, (int)c.n_strips);
  };
  if (smooth) {
    float4 *part = static_cast<float4 *>(c.part);
    with_vec<Tile>(a.nodes, a.d, [&](auto vec) { strip(strip_lse_smooth_kernel<Tile, decltype(vec)::value>, part); });
    hipLaunchKernelGGL(lse_smooth_merge_kernel, merge_grid, dim3(WG), 0, c.st, (const float4 *)part, (int)(2 * c.n_strips), Q, lse, ssum, (int *)cnt);
  } else {
    float2 *part = static_cast<float2 *>(c.part);
    with_vec<Tile>(a.nodes, a.d, [&](auto vec) { strip(strip_lse_kernel<Tile, decltype(vec)::value>, part); });
    hipLaunchKernelGGL(lse_merge_kernel, merge_grid, dim3(WG), 0, c.st, (const float2 *)part, (int)(2 * c.n_strips), Q, lse);
  }
  HIP_TRY(hipGetLastError());
  return RGCN_OK;
}

// the workspace of a gradient-cell call: strip_layout without partials, the mask as wide as the chunk
inline int64_t softmax_grad_workspace_bytes(int64_t Q, int64_t c_count, int32_t d, bool bf16) {
  return (Q < 0 || c_count <= 0 || d <= 0) ? 0 : strip_layout(Q, c_count, d, 0, bf16, 0).total;
}

}  // namespace

extern "C" int64_t rgcn_distmult_lse_workspace_bytes(int64_t Q, int64_t n_nodes, int32_t d, int32_t strips, int32_t bf16) {
  return (Q < 0 || n_nodes <= 0 || d <= 0 || strips < 0) ? 0 : strip_layout(Q, n_nodes, d, strips, bf16 != 0, sizeof(float2)).total;
}

extern "C" int rgcn_distmult_lse_f32(const int64_t *batch, int64_t Q, int32_t head, const float *nodes, const float *rel,
                                     const float *sbias, const float *pbias, const float *obias, const int32_t *filt_q,
                                     const int32_t *filt_n, int64_t F, const int64_t *fkeys, const int64_t *fptr, const int32_t *fvals,
                                     int64_t K, int32_t strips, void *workspace, float *lse, float *tscore, int64_t n_nodes, int32_t n_rel,
                                     int32_t d, void *stream) {
  (void)n_rel;
  return lse_fused<TileF32>({"distmult_lse", batch, Q, head, nodes, rel, sbias, pbias, obias, filt_q, filt_n, F, strips, workspace, n_nodes,
                             d, stream, filter_index(fkeys, fptr, fvals, K)}, lse, tscore);
}

extern "C" int rgcn_distmult_lse_bf16(const int64_t *batch, int64_t Q, int32_t head, const uint16_t *nodes, const float *rel,
                                      const float *sbias, const float *pbias, const float *obias, const int32_t *filt_q,
                                      const int32_t *filt_n, int64_t F, const int64_t *fkeys, const int64_t *fptr, const int32_t *fvals,
                                      int64_t K, int32_t strips, void *workspace, float *lse, float *tscore, int64_t n_nodes, int32_t n_rel,
                                      int32_t d, void *stream) {
  (void)n_rel;
  return lse_fused<TileBf16>({"distmult_lse_bf16", batch, Q, head, nodes, rel, sbias, pbias, obias, filt_q, filt_n, F, strips, workspace,
                              n_nodes, d, stream, filter_index(fkeys, fptr, fvals, K)}, lse, tscore);
}

// label smoothing: both storages again with ssum and cnt behind tscore, four floats per cell of the partials
extern "C" int64_t rgcn_distmult_lse_smooth_workspace_bytes(int64_t Q, int64_t n_nodes, int32_t d, int32_t strips, int32_t bf16) {
  return (Q < 0 || n_nodes <= 0 || d <= 0 || strips < 0) ? 0 : strip_layout(Q, n_nodes, d, strips, bf16 != 0, sizeof(float4)).total;
}

extern "C" int rgcn_distmult_lse_smooth_f32(const int64_t *batch, int64_t Q, int32_t head, const float *nodes, const float *rel,
                                            const float *sbias, const float *pbias, const float *obias, const int32_t *filt_q,
                                            const int32_t *filt_n, int64_t F, const int64_t *fkeys, const int64_t *fptr,
                                            const int32_t *fvals, int64_t K, int32_t strips, void *workspace, float *lse, float *tscore,
                                            float *ssum, int32_t *cnt, int64_t n_nodes, int32_t n_rel, int32_t d, void *stream) {
  (void)n_rel;
  return lse_fused<TileF32>({"distmult_lse_smooth", batch, Q, head, nodes, rel, sbias, pbias, obias, filt_q, filt_n, F, strips, workspace,
                             n_nodes, d, stream, filter_index(fkeys, fptr, fvals, K)}, lse, tscore, true, ssum, cnt);
}

extern "C" int rgcn_distmult_lse_smooth_bf16(const int64_t *batch, int64_t Q, int32_t head, const uint16_t *nodes, const float *rel,
                                             const float *sbias, const float *pbias, const float *obias, const int32_t *filt_q,
                                             const int32_t *filt_n, int64_t F, const int64_t *fkeys, const int64_t *fptr,
                                             const int32_t *fvals, int64_t K, int32_t strips, void *workspace, float *lse, float *tscore,
                                             float *ssum, int32_t *cnt, int64_t n_nodes, int32_t n_rel, int32_t d, void *stream) {
  (void)n_rel;
  return lse_fused<TileBf16>({"distmult_lse_smooth_bf16", batch, Q, head, nodes, rel, sbias, pbias, obias, filt_q, filt_n, F, strips,
                              workspace, n_nodes, d, stream, filter_index(fkeys, fptr, fvals, K)}, lse, tscore, true, ssum, cnt);
}

extern "C" int64_t rgcn_distmult_softmax_grad_workspace_bytes(int64_t Q, int64_t c_count, int32_t d, int32_t bf16) {
  return softmax_grad_workspace_bytes(Q, c_count, d, bf16 != 0);
}

namespace {

// the gradient cells of both storages, plain and smoothed: a.F fills the chunk's mask from the lists, a.ix.K from the index
template <class Tile>
int softmax_grad(const StripArgs<typename Tile::elem> &a, const float *lse, const float *gscale, int32_t per_query, int64_t mean_over, int64_t c_first,
                 int64_t c_count, float *dS, bool smooth = false, const float *keep = nullptr, const float *uni = nullptr) {
  const bool bad_chunk = c_first < 0 || c_first % 128 || c_count <= 0 || c_first > a.n_nodes - c_count || mean_over < 1;
  const float inv_q = 1.0f / (float)mean_over;
  if (smooth && (!keep || !uni)) { rgcn_set_error("%s: keep [1] and uni [Q] must be device pointers, not NULL", a.name); return RGCN_EINVAL; }
  if (int rc = strip_check(a, bad_chunk || (a.Q && (!lse || !gscale || !dS)), "c_first a multiple of 128, the chunk inside [0, n_nodes), mean_over >= 1; ")) return rc;
  if (a.Q == 0) return RGCN_OK;
  const int64_t nwg = ((c_count + 127) / 128) * ((a.Q + 127) / 128);
  if (nwg > INT32_MAX) { rgcn_set_error("%s: too many cells in one call; take a smaller chunk", a.name); return RGCN_EUNSUPPORTED; }
  StripCall<Tile> c;
  if (int rc = query_begin<Tile>(a, 0, 0, true, c_first, c_count, c)) return rc;       // no partials, keep_target = 0, the chunk's own mask
  auto launch = [&](auto vec, auto sm) {
    hipLaunchKernelGGL((softmax_grad_kernel<Tile, decltype(vec)::value, decltype(sm)::value>), dim3((unsigned)nwg), dim3(WG), 0, c.st, c.q, a.nodes,
                       c.dm, c.qb, c.cbias, c.b, lse, gscale, (int)per_query, inv_q, keep, uni, c.mask, (long long)c.mask_w, dS, (int)a.Q,
                       (long long)a.n_nodes, (long long)c_first, (long long)c_count, a.dir(), (int)c.qbl);
  };
  with_vec<Tile>(a.nodes, a.d, [&](auto vec) {
    if (smooth) launch(vec, std::true_type{}); else launch(vec, std::false_type{});
  });
  HIP_TRY(hipGetLastError());
  return RGCN_OK;
}

}  // namespace

extern "C" int rgcn_distmult_softmax_grad_f32(const int64_t *batch, int64_t Q, int32_t head, const float *nodes, const float *rel,
                                              const float *sbias, const float *pbias, const float *obias, const int32_t *filt_q,
                                              const int32_t *filt_n, int64_t F, const int64_t *fkeys, const int64_t *fptr,
                                              const int32_t *fvals, int64_t K, const float *lse, const float *gscale, int32_t per_query,
                                              int64_t mean_over, int64_t c_first, int64_t c_count, void *workspace, float *dS,
                                              int64_t n_nodes, int32_t n_rel, int32_t d, void *stream) {
  (void)n_rel;
  return softmax_grad<TileF32>({"distmult_softmax_grad", batch, Q, head, nodes, rel, sbias, pbias, obias, filt_q, filt_n, F, 0, workspace,
                                n_nodes, d, stream, filter_index(fkeys, fptr, fvals, K)}, lse, gscale, per_query, mean_over, c_first,
                                c_count, dS);
}

extern "C" int rgcn_distmult_softmax_grad_bf16(const int64_t *batch, int64_t Q, int32_t head, const uint16_t *nodes, const float *rel,
                                               const float *sbias, const float *pbias, const float *obias, const int32_t *filt_q,
                                               const int32_t *filt_n, int64_t F, const int64_t *fkeys, const int64_t *fptr,
                                               const int32_t *fvals, int64_t K, const float *lse, const float *gscale, int32_t per_query,
                                               int64_t mean_over, int64_t c_first, int64_t c_count, void *workspace, float *dS,
                                               int64_t n_nodes, int32_t n_rel, int32_t d, void *stream) {
  (void)n_rel;
  return softmax_grad<TileBf16>({"distmult_softmax_grad_bf16", batch, Q, head, nodes, rel, sbias, pbias, obias, filt_q, filt_n, F, 0,
                                 workspace, n_nodes, d, stream, filter_index(fkeys, fptr, fvals, K)}, lse, gscale, per_query, mean_over,
                                 c_first, c_count, dS);
}

// label smoothing: both storages again with keep [1] and uni [Q] behind gscale, the smoothed instantiation of the cell kernel
extern "C" int rgcn_distmult_softmax_grad_smooth_f32(const int64_t *batch, int64_t Q, int32_t head, const float *nodes, const float *rel,
                                                     const float *sbias, const float *pbias, const float *obias, const int32_t *filt_q,
                                                     const int32_t *filt_n, int64_t F, const int64_t *fkeys, const int64_t *fptr,
                                                     const int32_t *fvals, int64_t K, const float *lse, const float *gscale,
                                                     const float *keep, const float *uni, int32_t per_query, int64_t mean_over,
                                                     int64_t c_first, int64_t c_count, void *workspace, float *dS, int64_t n_nodes,
                                                     int32_t n_rel, int32_t d, void *stream) {
  (void)n_rel;
  return softmax_grad<TileF32>({"distmult_softmax_grad_smooth", batch, Q, head, nodes, rel, sbias, pbias, obias, filt_q, filt_n, F, 0,
                                workspace, n_nodes, d, stream, filter_index(fkeys, fptr, fvals, K)}, lse, gscale, per_query, mean_over,
                                c_first, c_count, dS, true, keep, uni);
}

extern "C" int rgcn_distmult_softmax_grad_smooth_bf16(const int64_t *batch, int64_t Q, int32_t head, const uint16_t *nodes,
                                                      const float *rel, const float *sbias, const float *pbias, const float *obias,
                                                      const int32_t *filt_q, const int32_t *filt_n, int64_t F, const int64_t *fkeys,
                                                      const int64_t *fptr, const int32_t *fvals, int64_t K, const float *lse,
                                                      const float *gscale, const float *keep, const float *uni, int32_t per_query,
                                                      int64_t mean_over, int64_t c_first, int64_t c_count, void *workspace, float *dS,
                                                      int64_t n_nodes, int32_t n_rel, int32_t d, void *stream) {
  (void)n_rel;
  return softmax_grad<TileBf16>({"distmult_softmax_grad_smooth_bf16", batch, Q, head, nodes, rel, sbias, pbias, obias, filt_q, filt_n, F, 0,
                                 workspace, n_nodes, d, stream, filter_index(fkeys, fptr, fvals, K)}, lse, gscale, per_query, mean_over,
                                 c_first, c_count, dS, true, keep, uni);
}

// ------------------------------------------------------------------ 1-N multi-label BCE loss: entry points
namespace {

// the mask is the label matrix: keep_target = 1 (a listed target stays set) and labels = true (the mask always exists, every query's own
// target set in it) -- whether the lists, the index or neither names the positives
template <class Tile>
int bce_sums(const StripArgs<typename Tile::elem> &a, float *sp, float *ps, int32_t *npos) {
  if (int rc = strip_check(a, a.Q && (!sp || !ps || !npos), "")) return rc;
  if (a.Q == 0) return RGCN_OK;
  StripCall<Tile> c;
  auto too_many = [&](int64_t) { return a.n_nodes > INT32_MAX; };     // npos counts a query's positive entities in 32 bits
  if (int rc = strip_begin<Tile>(a, sizeof(float4), 1, too_many, "entities", c, true)) return rc;
  float4 *part = static_cast<float4 *>(c.part);
  const int Q = (int)a.Q;
  with_vec<Tile>(a.nodes, a.d, [&](auto vec) {
    hipLaunchKernelGGL((strip_bce_kernel<Tile, decltype(vec)::value>), dim3((unsigned)(c.n_strips * c.qbl)), dim3(WG), 0, c.st, c.q, a.nodes, c.dm,
                       c.qb, c.cbias, c.mask, (long long)c.mask_w, part, Q, (long long)a.n_nodes, a.dir(), (int)c.qbl, (int)c.n_strips);
  });
  hipLaunchKernelGGL(bce_merge_kernel, dim3((unsigned)((a.Q + WG - 1) / WG)), dim3(WG), 0, c.st, (const float4 *)part, (int)(2 * c.n_strips), Q,
                     sp, ps, (int *)npos);
  HIP_TRY(hipGetLastError());
  return RGCN_OK;
}

// smooth: HOST floats {keep, uni} = {1 - eps, eps / n_nodes}, NULL = {1, 0}; they travel as kernel arguments
template <class Tile>
int bce_grad(const StripArgs<typename Tile::elem> &a, const float *gscale, int32_t per_query, int64_t mean_over, const float *smooth,
             int64_t c_first, int64_t c_count, float *dS) {
  const bool bad_chunk = c_first < 0 || c_first % 128 || c_count <= 0 || c_first > a.n_nodes - c_count || mean_over < 1;
  if (int rc = strip_check(a, bad_chunk || (a.Q && (!gscale || !dS)), "c_first a multiple of 128, the chunk inside [0, n_nodes), mean_over >= 1; ")) return rc;
  if (a.Q == 0) return RGCN_OK;
  const int64_t nwg = ((c_count + 127) / 128) * ((a.Q + 127) / 128);
  if (nwg > INT32_MAX) { rgcn_set_error("%s: too many cells in one call; take a smaller chunk", a.name); return RGCN_EUNSUPPORTED; }
  const float inv = (float)(1.0 / ((double)a.n_nodes * (double)mean_over));
  const float keep = smooth ? smooth[0] : 1.f, uni = smooth ? smooth[1] : 0.f;
  StripCall<Tile> c;
  if (int rc = query_begin<Tile>(a, 0, 1, true, c_first, c_count, c, true)) return rc;  // no partials, the chunk's own label mask
  with_vec<Tile>(a.nodes, a.d, [&](auto vec) {
    hipLaunchKernelGGL((bce_grad_kernel<Tile, decltype(vec)::value>), dim3((unsigned)nwg), dim3(WG), 0, c.st, c.q, a.nodes, c.dm, c.qb, c.cbias,
                       gscale, (int)per_query, inv, keep, uni, c.mask, (long long)c.mask_w, dS, (int)a.Q, (long long)a.n_nodes,
                       (long long)c_first, (long long)c_count, a.dir(), (int)c.qbl);
  });
  HIP_TRY(hipGetLastError());
  return RGCN_OK;
}

}  // namespace

extern "C" int64_t rgcn_distmult_bce_sums_workspace_bytes(int64_t Q, int64_t n_nodes, int32_t d, int32_t strips, int32_t bf16) {
  return (Q < 0 || n_nodes <= 0 || d <= 0 || strips < 0) ? 0 : strip_layout(Q, n_nodes, d, strips, bf16 != 0, sizeof(float4)).total;
}

extern "C" int64_t rgcn_distmult_bce_grad_workspace_bytes(int64_t Q, int64_t c_count, int32_t d, int32_t bf16) {
  return softmax_grad_workspace_bytes(Q, c_count, d, bf16 != 0);
}

extern "C" int rgcn_distmult_bce_sums_f32(const int64_t *batch, int64_t Q, int32_t head, const float *nodes, const float *rel,
                                          const float *sbias, const float *pbias, const float *obias, const int32_t *filt_q,
                                          const int32_t *filt_n, int64_t F, const int64_t *fkeys, const int64_t *fptr, const int32_t *fvals,
                                          int64_t K, int32_t strips, void *workspace, float *sp, float *ps, int32_t *npos, int64_t n_nodes,
                                          int32_t n_rel, int32_t d, void *stream) {
  (void)n_rel;
  return bce_sums<TileF32>({"distmult_bce_sums", batch, Q, head, nodes, rel, sbias, pbias, obias, filt_q, filt_n, F, strips, workspace, n_nodes, d,
                            stream, filter_index(fkeys, fptr, fvals, K)}, sp, ps, npos);
}

extern "C" int rgcn_distmult_bce_sums_bf16(const int64_t *batch, int64_t Q, int32_t head, const uint16_t *nodes, const float *rel,
                                           const float *sbias, const float *pbias, const float *obias, const int32_t *filt_q,
                                           const int32_t *filt_n, int64_t F, const int64_t *fkeys, const int64_t *fptr, const int32_t *fvals,
                                           int64_t K, int32_t strips, void *workspace, float *sp, float *ps, int32_t *npos, int64_t n_nodes,
                                           int32_t n_rel, int32_t d, void *stream) {
  (void)n_rel;
  return bce_sums<TileBf16>({"distmult_bce_sums_bf16", batch, Q, head, nodes, rel, sbias, pbias, obias, filt_q, filt_n, F, strips, workspace,
                             n_nodes, d, stream, filter_index(fkeys, fptr, fvals, K)}, sp, ps, npos);
}

extern "C" int rgcn_distmult_bce_grad_f32(const int64_t *batch, int64_t Q, int32_t head, const float *nodes, const float *rel,
                                          const float *sbias, const float *pbias, const float *obias, const int32_t *filt_q,
                                          const int32_t *filt_n, int64_t F, const int64_t *fkeys, const int64_t *fptr, const int32_t *fvals,
                                          int64_t K, const float *gscale, int32_t per_query, int64_t mean_over, const float *smooth,
                                          int64_t c_first, int64_t c_count, void *workspace, float *dS, int64_t n_nodes, int32_t n_rel,
                                          int32_t d, void *stream) {
  (void)n_rel;
  return bce_grad<TileF32>({"distmult_bce_grad", batch, Q, head, nodes, rel, sbias, pbias, obias, filt_q, filt_n, F, 0, workspace, n_nodes, d,
                            stream, filter_index(fkeys, fptr, fvals, K)}, gscale, per_query, mean_over, smooth, c_first, c_count, dS);
}

extern "C" int rgcn_distmult_bce_grad_bf16(const int64_t *batch, int64_t Q, int32_t head, const uint16_t *nodes, const float *rel,
                                           const float *sbias, const float *pbias, const float *obias, const int32_t *filt_q,
                                           const int32_t *filt_n, int64_t F, const int64_t *fkeys, const int64_t *fptr, const int32_t *fvals,
                                           int64_t K, const float *gscale, int32_t per_query, int64_t mean_over, const float *smooth,
                                           int64_t c_first, int64_t c_count, void *workspace, float *dS, int64_t n_nodes, int32_t n_rel,
                                           int32_t d, void *stream) {
  (void)n_rel;
  return bce_grad<TileBf16>({"distmult_bce_grad_bf16", batch, Q, head, nodes, rel, sbias, pbias, obias, filt_q, filt_n, F, 0, workspace, n_nodes,
                             d, stream, filter_index(fkeys, fptr, fvals, K)}, gscale, per_query, mean_over, smooth, c_first, c_count, dS);
}

// ------------------------------------------------------------------ device-resident filter index: the mask and the materialised route
extern "C" int rgcn_filter_mask_index(const int64_t *batch, int64_t Q, int32_t head, const int64_t *fkeys, const int64_t *fptr,
                                      const int32_t *fvals, int64_t K, int32_t keep_target, int64_t c_first, int64_t c_count, uint32_t *mask,
                                      int64_t n_nodes, void *stream) {
  const FilterIndexDev ix = filter_index(fkeys, fptr, fvals, K);
  if (Q < 0 || Q > INT32_MAX || n_nodes <= 0 || bad_index(ix) || c_first < 0 || c_count <= 0 || c_first > n_nodes - c_count ||
      (Q && (!batch || !mask))) {
    rgcn_set_error("filter_mask_index: bad argument (K > 0 needs keys, ptr and vals; the columns inside [0, n_nodes))");
    return RGCN_EINVAL;
  }
  if (bad_query_form("filter_mask_index", head, 0)) return RGCN_EINVAL;
  if (Q == 0) return RGCN_OK;
  const int64_t mask_w = (c_count + 31) / 32;
  hipStream_t st = (hipStream_t)stream;
  HIP_TRY(zero_async(mask, (size_t)(Q * mask_w) * sizeof(unsigned), st));
  if (K) launch_index_mask(st, mask, mask_w, ix, reinterpret_cast<const long long *>(batch), Q, query_dir(head), n_nodes, keep_target, c_first, c_first + c_count);
  HIP_TRY(hipGetLastError());
  return RGCN_OK;
}

extern "C" int rgcn_rank_filter_index_f32(float *scores, const int64_t *batch, int64_t Q, int32_t head, int64_t n_nodes, const int64_t *fkeys,
                                          const int64_t *fptr, const int32_t *fvals, int64_t K, int32_t keep_target, void *stream) {
  const FilterIndexDev ix = filter_index(fkeys, fptr, fvals, K);
  if (Q < 0 || Q > INT32_MAX || n_nodes <= 0 || bad_index(ix) || (Q && K && (!scores || !batch))) {
    rgcn_set_error("rank_filter_index: bad argument");
    return RGCN_EINVAL;
  }
  if (bad_query_form("rank_filter_index", head, 0)) return RGCN_EINVAL;
  if (K == 0 || Q == 0) return RGCN_OK;
  hipLaunchKernelGGL(index_filter_kernel, dim3((unsigned)((Q + WG / 64 - 1) / (WG / 64))), dim3(WG), 0, (hipStream_t)stream, scores, ix,
                     reinterpret_cast<const long long *>(batch), (int)Q, query_dir(head), (long long)n_nodes, keep_target);
  HIP_TRY(hipGetLastError());
  return RGCN_OK;
}
