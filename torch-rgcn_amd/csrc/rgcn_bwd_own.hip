// Relation-owner backward of the hidden-16 relational layer on TALL tiles in soft-window order (round 6).
//
// Autograd duals of reference torch_rgcn/layers.py:293-301, one random row gather per message:
//     dX[o]  += val * G[s] W_r^T            dW_r += val * X[o]^T G[s]            for every message (s <- o, r, val)
//
// Why another form.  The gather of S1's 21 M rows takes 0.375 ms in random order and 0.19-0.22 ms when the whole chip reads from a few MB
// of the table at any time (tools/micro/gather_window.hip).  The plan gives that order for free when a (tile, relation) bucket holds many
// chunks (_native.build_softwin_plan: buckets sorted by source, a tile's chunks ordered by first source) -- which wants tiles of ~1000
// rows, and the block-tile kernel (rgcn_bwd_blk.hip) holds 218: its LDS keeps every relation's dW (R KiB) next to the X and dX tiles.
// Here dW sits in REGISTERS.  Every relation -- every part of a large one -- belongs to one of the workgroup's NW waves (LPT over the
// message counts, made with the plan); a wave walks only the chunks of its units and keeps their K accumulators (the MFMA's 16 x 16 D
// fragment: 4 registers each) as K separate register quads; wave-uniform tests of the chunk's local number pick the case whose four
// MFMAs name that quad, so the dW products accumulate in place under compile-time register numbers (no s_set_gpr_idx_on / indexed
// v_mov: -0.009 ms per launch at S1).  No LDS table, no compare-and-swap adds, no dirty flags; the registers leave the
// CU once, at the end of the kernel (the same R KiB of global atomics per workgroup as the block-tile kernel's one flush).
// LDS = the dX tile in doubles (128 bytes per row, ds_add_f64 as in the block-tile kernel) + the X tile (64 bytes per row: A operand of
// the dW products, ReLU mask of the epilogue) + 1 KiB of transposition scratch per wave: tiles of up to 767 rows (S1: 652 rows, 1534
// tiles, 6 per CU; a bucket holds 135 messages = 8-9 chunks of ~8 MB source span).
// Shape: 16 waves x 8 units x 2 chunks per loop trip.  Measured at S1 (tools/r6_own_variants.sh, bench.py's per-launch
// average): 12 waves x 9 units x 4 chunks (152 VGPRs, the first shipped form) 0.460 ms; 16 x 7 x 4 (128 VGPRs, 11 spilled) 0.454;
// 16 x 8 x 3 0.437 -- the loads in flight per CU are the same 48 chunks, the fourth wave per SIMD hides the LDS and MFMA phases;
// 16 x 8 x 2 **0.432**, 16 x 8 x 1 0.447 (fewer chunks in flight narrow the span of sources the chip reads at one time).
// (Those forms kept the accumulators in one <32 x float> under a dynamic index; the ninth of the 12 x 9 form sat behind a select.)
// Measured and dropped on the way (tools/r6_own_abl.sh, profiles/r06_own_ablation.txt): the X rows read from global memory instead of an
// LDS tile (tiles of 977 rows fit then): 16 more loads per four chunks, +0.09 ms; accumulators updated by indexed adds: +0.03 ms.
//
// The chunk records are the block-tile kernel's (rgcn_bwd_blk_prepare_f32, 176 bytes); the relation word carries the local relation
// number in its high half: rel | li << 16.  own_ptr[tile * NW + wave] = first chunk of the wave in the tile (n_tiles * NW + 1 entries).
// Static plans whose fields fit come as PACKED records instead (96 bytes per chunk behind a dictionary of the plan's vals:
// rgcn_bwd_blk_prepare_packed_f32, rgcn_device.h, template parameter PK): S1 0.4000 -> 0.3878 ms per launch (profiles/packed_rec_*.txt);
// 116 VGPRs against 118 (bf16: 120 against 122), no scratch.
// Shared group (own_relations(shared=True)): the relation with the most messages -- S1: the self loops, 41 chunks per tile that gather the
// tile's own rows -- belongs to no wave; its chunks are group NW of a tile (group_ptr, NW + 1 groups per tile) and go, two at a time, to
// whichever wave is done with its own range, and the waves' sums of it leave the workgroup as ONE set of atomics.  S1: 0.4139 -> 0.4019 ms
// per launch against that relation cut into two owned parts.  Cutting relations to level the waves does not pay: every part is one more
// set of atomics per workgroup on the relation's 1 KiB of dW when the kernel ends (profiles/own_shared_*.txt).
// No hub pieces: plans with hub tiles keep the block-tile kernel.
#include <stdlib.h>
#include <string.h>

#include <algorithm>

#include "rgcn_device.h"

namespace {

constexpr int OWN_REC = 176;
constexpr int OWN_REC_ROWS = 128;
constexpr int OWN_REC_HDR = 160;
constexpr int OWN_LDS_MAX = 160 * 1024;
#ifndef RGCN_OWN_NW
#define RGCN_OWN_NW 16
#define RGCN_OWN_K 8
#define RGCN_OWN_U 2
#endif
constexpr int OWN_NW = RGCN_OWN_NW;  // waves per workgroup
constexpr int OWN_K = RGCN_OWN_K;    // relations per wave (accumulators in registers)
constexpr int OWN_U = RGCN_OWN_U;    // chunks per loop trip
constexpr int OWN_MAX_ROWS = (OWN_LDS_MAX - OWN_NW * BW_SCR2 * 4 - 64) / 192;      // 767: dX tile (doubles) + X tile + the waves' scratch

// One case of the accumulator selection: the chunk's four dW MFMAs on accumulator I, in place.  The cases are separate wave-uniform
// ifs, not the arms of one switch: the compiler structurizes a multiway branch into a chain of merge blocks that copy every
// accumulator of the other arms (v_mov blocks the size of the register vector); an if of its own names only its own four registers
// and its merge moves nothing.  (The empty asm keeps the optimizer from threading the ifs back into one multiway branch.)  Measured and
// not kept: the cases in groups of four behind a test of lr >> 2 (fewer branches per chunk, +0.002 ms per launch).
#define OWN_DW_CASE(I)                                                                                             \
  if constexpr (I < K) {                                                                                           \
    if (lr == I) {                                                                                                 \
      _Pragma("unroll") for (int t4 = 0; t4 < 4; ++t4)                                                             \
        accw[I] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t4], b[t4], accw[I], 0, 0, 0);                            \
    }                                                                                                              \
    asm volatile("" : "+s"(lr));                                                                                   \
  }

size_t bwd_own_lds(int rows, bool packed = false) { return (size_t)rows * 192 + (size_t)OWN_NW * BW_SCR2 * 4 + 64 + (packed ? PK_LDS : 0); }
constexpr int OWN_MAX_ROWS_PK = (OWN_LDS_MAX - OWN_NW * BW_SCR2 * 4 - 64 - PK_LDS) / 192;      // 762: the dictionary sits behind the counter

// Timing experiments (ablation library only, make abl; wrong results): ABL bits 2 no dW part, 8 no dX tile update, 16 loads only
// BF (rgcn_bwd_own_bf16): G, X and dX hold bf16 rows (32 bytes); G is gathered 8 bytes per lane (the record's byte offset
// src << 6 halved) and widened, the X tile in LDS stays fp32, dX is rounded once on the way out; dW and the bias gradient stay fp32.
// BF = false is the fp32 kernel as it was.
// PK: packed records (rgcn_bwd_blk_prepare_packed_f32, rgcn_device.h): two record loads per lane and chunk instead of three, the val from
// the dictionary's copy in LDS (PK_LDS bytes behind the counter), the header rel | local << 16 from lane 0's row words.  PK = false is
// the kernel on the wide records as it was.
template <bool RELU, int NW, int K, int ABL = 0, bool BF = false, bool PK = false>
__global__ __launch_bounds__(64 * NW) void bwd_own_d16_kernel(
    const float *__restrict__ G, const float *__restrict__ X, const float *__restrict__ Wtp, float *__restrict__ dX,
    float *__restrict__ dWout, const char *__restrict__ rec, const int *__restrict__ gptr, int gstride, int shared_rel, int n_tiles,
    int tile_rows, int n_dst, float *__restrict__ dbias, int n_src, const int *__restrict__ unit_rel) {
  constexpr int U = OWN_U, NT = 64 * NW;
  constexpr int TQ = (OWN_MAX_ROWS * 4 + NT - 1) / NT;            // float4 of a tile a thread carries / converts per tile, at most
  static_assert(K <= 9, "dw_add lists nine accumulator cases");
  extern __shared__ __attribute__((aligned(16))) char lds[];
  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  const unsigned xt_off = (unsigned)tile_rows * 128u;             // bytes: the dX tile [rows][16] doubles comes first
  const unsigned xs_off = (unsigned)tile_rows * 192u;
  float4 *dxz = reinterpret_cast<float4 *>(lds);
  const double2 *dxd2 = reinterpret_cast<const double2 *>(lds);
  float4 *xt4 = reinterpret_cast<float4 *>(lds + xt_off);         // X tile [rows][16] floats
  float *xs = reinterpret_cast<float *>(lds + xs_off) + wave * BW_SCR2;
  // The shared group (gstride = NW + 1 groups per tile, shared_rel >= 0): chunks of relation shared_rel that belong to no wave.  A wave whose
  // last slot names that relation takes them U at a time from a counter in LDS (the 64 spare bytes behind the scratch) once its own range
  // is done, so the waves reach the tile's barrier together; its sums sit in accumulator K - 1 (the chunks' local number).
  int *ctr = reinterpret_cast<int *>(lds + xs_off + (unsigned)NW * BW_SCR2 * 4u);
  const bool takes = shared_rel >= 0 && __builtin_amdgcn_readfirstlane(unit_rel[wave * K + K - 1]) == shared_rel;
  auto take = [&]() {
    int v = 0;
    if (lane == 0) v = __hip_atomic_fetch_add(ctr, U, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    return __builtin_amdgcn_readfirstlane(v);
  };
  // a tile's ranges: [a, b) this wave's own chunks, [sa, sb) the shared group (empty for a wave that does not take part)
  auto ranges = [&](int tt, int &a, int &b, int &sa, int &sb) {
    const int *g = gptr + (size_t)tt * gstride;
    a = __builtin_amdgcn_readfirstlane(g[wave]);
    b = __builtin_amdgcn_readfirstlane(g[wave + 1]);
    sa = sb = 0;
    if (takes) {
      sa = __builtin_amdgcn_readfirstlane(g[NW]);
      sb = __builtin_amdgcn_readfirstlane(g[NW + 1]);
    }
  };

  int t = blockIdx.x;
  int row0 = t * tile_rows;
  int nrows = min(tile_rows, n_dst - row0);
  int c0, c1, s0, s1;
  ranges(t, c0, c1, s0, s1);
  if (tid == 0) lds_st(ctr, 0);
  const float *dict = reinterpret_cast<const float *>(ctr + 16);      // PK: the val dictionary, entry PK_DICT = 0.0f
  if constexpr (PK)
    for (int i = tid; i <= PK_DICT; i += NT) ctr[16 + i] = i < PK_DICT ? reinterpret_cast<const int *>(rec)[i] : 0;
  float4 gs = make_float4(0.f, 0.f, 0.f, 0.f);
  const long long g_n4 = dbias ? (long long)n_src * 4 : 0, g_step = (long long)gridDim.x * NT;
  long long g_i = (long long)blockIdx.x * NT + tid;
#pragma unroll
  for (int q = 0; q < TQ; ++q) {
    const int idx = tid + q * NT;
    if (idx < tile_rows * 4) {
      float4 x0 = make_float4(0.f, 0.f, 0.f, 0.f);
      if (idx < nrows * 4) {
        if constexpr (BF) x0 = bf16x4_widen(reinterpret_cast<const uint2 *>(X)[(size_t)row0 * 4 + idx]);
        else x0 = reinterpret_cast<const float4 *>(X + (size_t)row0 * 16)[idx];
      }
      xt4[idx] = x0;
    }
  }
  for (int i = tid; i < tile_rows * 8; i += NT) dxz[i] = make_float4(0.f, 0.f, 0.f, 0.f);
  __syncthreads();

  const int m = lane & 15, k = lane >> 4;
  const unsigned kofs = (unsigned)k << 4;
  const unsigned dx_lane = (unsigned)m * 8u;                            // LDS byte address of dX tile [0][m]
  const unsigned xrd = xt_off + (unsigned)m * 4u;                       // LDS byte address of X tile [0][m]
  // scratch (as in the block-tile kernel): the float4 column (features 4c .. 4c+3) of slot s is stored at column (c + (s >> 2)) & 3
  float *xs_wr = xs + m * 16 + 4 * ((k + (m >> 2)) & 3);                // this lane's float4: features 4k .. 4k+3 of slot m
  const float *xs_rd = xs + (4 * k) * 16 + 4 * (((m >> 2) + k) & 3) + (m & 3);   // feature m of slot 4k + t: + 16 t
  const unsigned slot_lane = (unsigned)m * 8u;
  const unsigned rows_lane = (unsigned)OWN_REC_ROWS + (unsigned)k * 8u;
  const unsigned w_lane = (unsigned)lane * 16u;

  f32x4 accw[K];
#pragma unroll
  for (int i = 0; i < K; ++i) accw[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  // dW_unit += A^T B on the accumulator of local unit lr (wave-uniform, < K by the plan: own_relations gives a wave at most K units)
  auto dw_add = [&](int lr, const float (&a)[4], const float (&b)[4]) {
    OWN_DW_CASE(0) OWN_DW_CASE(1) OWN_DW_CASE(2) OWN_DW_CASE(3) OWN_DW_CASE(4) OWN_DW_CASE(5) OWN_DW_CASE(6) OWN_DW_CASE(7) OWN_DW_CASE(8)
  };

  uint2 sl_n[U], rw_n[U];
  int hd_n[U];
  auto request_idx = [&](int c, int last) {
#pragma unroll
    for (int j = 0; j < U; ++j) {
      const int cc = min(c + j, last);                          // scalar: chunks past the wave's range re-read its last chunk (val forced to 0)
      if constexpr (PK) {       // the slot word of slot m, the four row words of quarter k (lane 0's carry the header)
        const char *r = rec + PK_DICT_BYTES + (size_t)cc * PK_REC;
        sl_n[j].x = *reinterpret_cast<const unsigned *>(r + (unsigned)m * 4u);
        rw_n[j] = *reinterpret_cast<const uint2 *>(r + ((unsigned)PK_REC_ROWS + (unsigned)k * 8u));
      } else {
      const char *r = rec + (size_t)cc * OWN_REC;
      sl_n[j] = *reinterpret_cast<const uint2 *>(r + slot_lane);
      rw_n[j] = *reinterpret_cast<const uint2 *>(r + rows_lane);
      hd_n[j] = *reinterpret_cast<const int *>(r + OWN_REC_HDR);
      }
    }
  };
  if (c0 < c1) request_idx(c0, c1 - 1);

  for (;;) {
    // the wave's pairs of this tile: its own range (the first pair was requested a tile ago), then what the counter deals it
    int c = c0, last = c1 - 1;
    bool sh = false;
    if (c > last && s0 < s1) {
      sh = true;
      c = s0 + take();
      last = s1 - 1;
      if (c <= last) request_idx(c, last);
    }
    while (c <= last) {
      unsigned w0_[U];
      uint2 rw_[U];
      float v_[U];
      int hd_[U];
      float4 g_[U], w_[U];
#pragma unroll
      for (int j = 0; j < U; ++j) {
        if constexpr (PK) {       // src << 8 | code -> src << 6; the val's LDS read is issued here and awaited at the products
          w0_[j] = (sl_n[j].x >> 2) & 0xFFFFFFC0u;
          rw_[j] = rw_n[j];
          v_[j] = dict[(c + j <= last) ? sl_n[j].x & 0xFFu : (unsigned)PK_DICT];
          hd_[j] = pk_header(__builtin_amdgcn_readfirstlane(rw_n[j].x), __builtin_amdgcn_readfirstlane(rw_n[j].y));
        } else {
        w0_[j] = sl_n[j].x;
        rw_[j] = rw_n[j];
        v_[j] = (c + j <= last) ? __builtin_bit_cast(float, sl_n[j].y) : 0.f;
        hd_[j] = __builtin_amdgcn_readfirstlane(hd_n[j]);
        }
      }
      if constexpr (PK) {
#pragma unroll
        for (int j = 0; j < U; ++j) asm volatile("" : "+v"(w0_[j]));
      } else {
#pragma unroll
      for (int j = 0; j < U; ++j) asm volatile("" : "+v"(w0_[j]), "+v"(v_[j]));   // pin the index data here
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int j = 0; j < U; ++j) {
        if constexpr (BF) {
          g_[j] = bf16x4_widen(*reinterpret_cast<const uint2 *>(reinterpret_cast<const char *>(G) + ((w0_[j] >> 1) | (kofs >> 1))));
        } else {
          const unsigned og = w0_[j] | kofs;
          g_[j] = *reinterpret_cast<const float4 *>(reinterpret_cast<const char *>(G) + og);
        }
        w_[j] = *reinterpret_cast<const float4 *>(reinterpret_cast<const char *>(Wtp) + (size_t)(hd_[j] & 0xFFFF) * 1024 + w_lane);
      }
      __builtin_amdgcn_sched_barrier(0);
      {     // the pair after this one, requested a trip ahead: the next of the own range, else the next the counter hands out
        int cn = c + U, lastn = last;
        if (sh || (cn > last && s0 < s1)) {
          sh = true;
          cn = s0 + take();
          lastn = s1 - 1;
        }
        if (cn <= lastn) request_idx(cn, lastn);
        c = cn;
        last = lastn;
      }
      __builtin_amdgcn_sched_barrier(0);
      if (ABL & 16) {
#pragma unroll
        for (int j = 0; j < U; ++j) asm volatile("" :: "v"(g_[j].x), "v"(g_[j].y), "v"(g_[j].z), "v"(g_[j].w), "v"(w_[j].x), "v"(w_[j].w), "v"(rw_[j].x), "v"(rw_[j].y), "v"(v_[j]));
        continue;
      }
      // ---- phase 1: scaled rows, dX products (four independent MFMA chains): D[slot][o], lane (k, m) <- slots 4k .. 4k+3, feature m
      f32x4 sc[U], acc[U];
#pragma unroll
      for (int j = 0; j < U; ++j) {
        sc[j] = f32x4{g_[j].x * v_[j], g_[j].y * v_[j], g_[j].z * v_[j], g_[j].w * v_[j]};
        acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
      }
#pragma unroll
      for (int j = 0; j < U; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(sc[j][0], w_[j].x, acc[j], 0, 0, 0);
#pragma unroll
      for (int j = 0; j < U; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(sc[j][1], w_[j].y, acc[j], 0, 0, 0);
#pragma unroll
      for (int j = 0; j < U; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(sc[j][2], w_[j].z, acc[j], 0, 0, 0);
#pragma unroll
      for (int j = 0; j < U; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(sc[j][3], w_[j].w, acc[j], 0, 0, 0);
      // tile rows of slots 4k .. 4k+3 (the records hold them x 64: the byte offset of the X row)
      unsigned ro[U][4];
#pragma unroll
      for (int j = 0; j < U; ++j) {
        ro[j][0] = rw_[j].x & 0xFFFFu;
        ro[j][1] = rw_[j].x >> 16;
        ro[j][2] = rw_[j].y & 0xFFFFu;
        ro[j][3] = rw_[j].y >> 16;
        if constexpr (PK) {       // (the low 6 bits of a row word may hold header bits)
#pragma unroll
          for (int e = 0; e < 4; ++e) ro[j][e] &= 0xFFC0u;
        }
      }
      // ---- phase 2: dW products, two chunks at a time: the scaled rows go through the wave's scratch into K-over-messages layout, the
      // X rows of the slots come from the X tile; the products accumulate IN the wave's register accumulator of the chunk's relation
#pragma unroll
      for (int h = 0; h < U && !(ABL & 2); h += 2) {
        constexpr int P = 2;
        float bv[P][4], av[P][4];
#pragma unroll
        for (int jj = 0; jj < P; ++jj) {
          const int j = h + jj;
          if (j >= U) break;
          asm volatile("" ::: "memory");
          *reinterpret_cast<f32x4 *>(xs_wr) = sc[j];
          asm volatile("" ::: "memory");
#pragma unroll
          for (int t4 = 0; t4 < 4; ++t4) bv[jj][t4] = xs_rd[16 * t4];
#pragma unroll
          for (int t4 = 0; t4 < 4; ++t4) av[jj][t4] = *reinterpret_cast<const float *>(lds + (xrd + ro[j][t4]));
          asm volatile("" ::: "memory");
        }
        // (two chunks of one pair may share their unit: the second dw_add runs after the first and reads what it wrote)
#pragma unroll
        for (int jj = 0; jj < P; ++jj) {
          if (h + jj >= U) break;
          dw_add((int)((unsigned)hd_[h + jj] >> 16), av[jj], bv[jj]);
        }
      }
      // ---- phase 3: the tile update, one ds_add_f64 per slot quarter: the 16 lanes of a quarter wave add to the 16 features of one row
#pragma unroll
      for (int j = 0; j < U && !(ABL & 8); ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e)
          __hip_atomic_fetch_add(static_cast<double *>(__builtin_assume_aligned(lds + (dx_lane + 2u * ro[j][e]), 8)), (double)acc[j][e], __ATOMIC_RELAXED,
                                 __HIP_MEMORY_SCOPE_WORKGROUP);
      __builtin_amdgcn_sched_barrier(0);
    }
    // the next tile of this workgroup: its X rows, this wave's first chunks and one float4 of G (bias gradient) are requested before the barrier
    const int tn = t + (int)gridDim.x;
    int c0n = 0, c1n = 0, s0n = 0, s1n = 0, row0n = 0, nrn = 0;
    float4 xn[TQ];
#pragma unroll
    for (int q = 0; q < TQ; ++q) xn[q] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (tn < n_tiles) {
      row0n = tn * tile_rows;
      nrn = min(tile_rows, n_dst - row0n);
      ranges(tn, c0n, c1n, s0n, s1n);
#pragma unroll
      for (int q = 0; q < TQ; ++q)
        if (tid + q * NT < nrn * 4) {
          if constexpr (BF) {     // (the raw bf16 bits ride in .x / .y across the barrier, widened when the tile is installed)
            const uint2 u = reinterpret_cast<const uint2 *>(X)[(size_t)row0n * 4 + tid + q * NT];
            xn[q] = make_float4(__uint_as_float(u.x), __uint_as_float(u.y), 0.f, 0.f);
          } else {
            xn[q] = reinterpret_cast<const float4 *>(X + (size_t)row0n * 16)[tid + q * NT];
          }
        }
      if (c0n < c1n) request_idx(c0n, c1n - 1);
    }
    float4 gn = make_float4(0.f, 0.f, 0.f, 0.f);
    if (g_i < g_n4) {
      if constexpr (BF) gn = bf16x4_widen(reinterpret_cast<const uint2 *>(G)[g_i]);
      else gn = reinterpret_cast<const float4 *>(G)[g_i];
    }
    g_i += g_step;
    lds_barrier();                                                 // every wave has finished adding to the dX tile
    gs.x += gn.x; gs.y += gn.y; gs.z += gn.z; gs.w += gn.w;
    // (what was requested before the barrier is pinned as arrived BEFORE the tile's stores: vmcnt counts in order)
#pragma unroll
    for (int q = 0; q < TQ; ++q) asm volatile("" : "+v"(xn[q].x), "+v"(xn[q].y), "+v"(xn[q].z), "+v"(xn[q].w));
#pragma unroll
    for (int q = 0; q < TQ; ++q) {
      const int idx = tid + q * NT;
      if (idx < nrows * 4) {
        const double2 d0 = dxd2[2 * idx], d1 = dxd2[2 * idx + 1];
        float4 a = make_float4((float)d0.x, (float)d0.y, (float)d1.x, (float)d1.y);
        if (RELU) {
          const float4 x = xt4[idx];
          a.x = x.x > 0.f ? a.x : 0.f; a.y = x.y > 0.f ? a.y : 0.f; a.z = x.z > 0.f ? a.z : 0.f; a.w = x.w > 0.f ? a.w : 0.f;
        }
        if constexpr (BF) reinterpret_cast<uint2 *>(dX)[(size_t)row0 * 4 + idx] = bf16x4_round(a);
        else reinterpret_cast<float4 *>(dX + (size_t)row0 * 16)[idx] = a;
      }
    }
    if (tn >= n_tiles) break;
    if (tid == 0) lds_st(ctr, 0);                                  // (between the barriers: nobody takes from it)
#pragma unroll
    for (int q = 0; q < TQ; ++q) {
      const int idx = tid + q * NT;
      if (idx < tile_rows * 4) {
        dxz[2 * idx] = make_float4(0.f, 0.f, 0.f, 0.f);
        dxz[2 * idx + 1] = make_float4(0.f, 0.f, 0.f, 0.f);
        if constexpr (BF) xt4[idx] = bf16x4_widen(uint2{__float_as_uint(xn[q].x), __float_as_uint(xn[q].y)});
        else xt4[idx] = xn[q];
      }
    }
    lds_barrier();                                                 // the next tile is installed (nobody waits for the dX stores)
    t = tn; row0 = row0n; nrows = nrn; c0 = c0n; c1 = c1n; s0 = s0n; s1 = s1n;
  }
  if (dbias) {
    for (; g_i < g_n4; g_i += g_step) {
      float4 gn;
      if constexpr (BF) gn = bf16x4_widen(reinterpret_cast<const uint2 *>(G)[g_i]);
      else gn = reinterpret_cast<const float4 *>(G)[g_i];
      gs.x += gn.x; gs.y += gn.y; gs.z += gn.z; gs.w += gn.w;
    }
    // thread tid holds features 4 (tid & 3) .. + 3: fold the 16 lanes of a wave that share (lane & 3), then the waves through the scratch
#pragma unroll
    for (int sft = 4; sft < 64; sft <<= 1) {
      gs.x += __shfl_xor(gs.x, sft); gs.y += __shfl_xor(gs.y, sft); gs.z += __shfl_xor(gs.z, sft); gs.w += __shfl_xor(gs.w, sft);
    }
    __syncthreads();                                               // (every wave is done with its scratch)
    if (lane < 4) *reinterpret_cast<float4 *>(xs + 4 * lane) = gs;
    __syncthreads();
    if (tid < 16) {
      float a = 0.f;
      const float *all = reinterpret_cast<const float *>(lds + xs_off);
      for (int i = 0; i < NW; ++i) a += all[i * BW_SCR2 + tid];
      atomicAdd(dbias + tid, a);
    }
  }
  // the wave's accumulators leave the CU once.  D fragment: lane 16k + m, element e = row 4k + e (input feature), column m
  if (shared_rel >= 0) {     // the shared relation's NW accumulators: summed through the waves' scratch, one wave's atomics for the workgroup
    __syncthreads();                                               // (every wave is done with its scratch)
    *reinterpret_cast<f32x4 *>(xs + 4 * lane) = takes ? accw[K - 1] : f32x4{0.f, 0.f, 0.f, 0.f};
    __syncthreads();
    if (wave == 0) {
      const float *all = reinterpret_cast<const float *>(lds + xs_off) + 4 * lane;
      f32x4 a = f32x4{0.f, 0.f, 0.f, 0.f};
      for (int i = 0; i < NW; ++i) a += *reinterpret_cast<const f32x4 *>(all + i * BW_SCR2);
      float *o = dWout + (size_t)shared_rel * 256 + (4 * k) * 16 + m;
      atomicAdd(o, a[0]);
      atomicAdd(o + 16, a[1]);
      atomicAdd(o + 32, a[2]);
      atomicAdd(o + 48, a[3]);
    }
  }
#pragma unroll
  for (int li = 0; li < K; ++li) {
    const int r = __builtin_amdgcn_readfirstlane(unit_rel[wave * K + li]);
    if (r >= 0 && !(takes && li == K - 1)) {
      float *o = dWout + (size_t)r * 256 + (4 * k) * 16 + m;
      atomicAdd(o, accw[li][0]);
      atomicAdd(o + 16, accw[li][1]);
      atomicAdd(o + 32, accw[li][2]);
      atomicAdd(o + 48, accw[li][3]);
    }
  }
}

#undef OWN_DW_CASE

}  // namespace

extern "C" int32_t rgcn_bwd_own_waves(void) { return OWN_NW; }
extern "C" int32_t rgcn_bwd_own_units(void) { return OWN_NW * OWN_K; }
extern "C" int32_t rgcn_bwd_own_max_rows(void) { return OWN_MAX_ROWS; }
// (defined here: the owner kernel's LDS budget is this file's; the forward takes packed records on every tile it takes at all)
extern "C" int32_t rgcn_bwd_blk_packed_max_rows(int32_t owner) { return owner ? OWN_MAX_ROWS_PK : rgcn_spmm_blk_max_rows(); }

// group_ptr / shared_rel of the two entries: the plan's pointer array with OWN_NW + 1 groups per tile and the shared relation, or NULL / -1
// (the kernel then walks own_ptr, OWN_NW groups per tile, and there is no shared group)
static bool own_groups_ok(const int32_t *own_ptr, const int32_t *group_ptr, int32_t shared_rel, int64_t n_tiles, int32_t R) {
  if (!group_ptr) return own_ptr && shared_rel < 0;
  return shared_rel >= 0 && shared_rel < R && n_tiles * (int64_t)(OWN_NW + 1) < INT32_MAX;
}

extern "C" int rgcn_bwd_own_f32(const float *G, const float *X, const float *Wt_packed, float *dX, float *dW, const void *rec,
                                const int32_t *own_ptr, const int32_t *group_ptr, int32_t shared_rel, const int32_t *unit_rel, int64_t n_tiles,
                                int32_t tile_rows, int64_t n_dst, int32_t R, int32_t flags, float *dbias, int64_t n_src, void *stream) {
  if (!G || !X || !Wt_packed || !dX || !dW || !rec || !unit_rel || n_tiles <= 0 || tile_rows <= 0 || n_dst <= 0 || R <= 0 ||
      R > 0xFFFF || n_dst > INT32_MAX || n_tiles * (int64_t)OWN_NW >= INT32_MAX || !own_groups_ok(own_ptr, group_ptr, shared_rel, n_tiles, R)) {
    rgcn_set_error("bwd_own: bad argument");
    return RGCN_EINVAL;
  }
  const bool packed = (flags & RGCN_F_PACKED_REC) != 0;
  if (tile_rows > (packed ? OWN_MAX_ROWS_PK : OWN_MAX_ROWS)) {
    rgcn_set_error("bwd_own: tiles of at most %d rows (got %d)", packed ? OWN_MAX_ROWS_PK : OWN_MAX_ROWS, tile_rows);
    return RGCN_EUNSUPPORTED;
  }
  if (n_src <= 0 || n_src >= (int64_t(1) << 26)) {
    rgcn_set_error("bwd_own: the records address G rows as src << 6 in 32 bits: 0 < n_src < 2^26");
    return RGCN_EINVAL;
  }
  hipStream_t st = (hipStream_t)stream;
  int dev = 0, n_cu = 0;
  HIP_TRY(launch_device(&dev, &n_cu));
  HIP_TRY(zero_dw_dbias_async(dW, (size_t)R, dbias, st));
  const size_t lds = bwd_own_lds(tile_rows, packed);
  const unsigned n_blocks = (unsigned)std::min<int64_t>(n_tiles, n_cu);
  auto launch = [&](auto k) -> hipError_t {
    constexpr auto kern = decltype(k)::value;
    hipError_t e = allow_lds<kern>(dev, lds, OWN_LDS_MAX);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, dim3(n_blocks), dim3(64 * OWN_NW), lds, st, G, X, Wt_packed, dX, dW, static_cast<const char *>(rec), group_ptr ? group_ptr : own_ptr,
                       group_ptr ? OWN_NW + 1 : OWN_NW, group_ptr ? shared_rel : -1, (int)n_tiles, tile_rows, (int)n_dst, dbias, (int)n_src, unit_rel);
    return hipGetLastError();
  };
#ifdef RGCN_ABLATIONS
  {
    const int ABLV = rgcn_option_value(RGCN_OPT_BWD_ABL);
    if (packed) { rgcn_set_error("bwd_own (ablation library): wide records only"); return RGCN_EUNSUPPORTED; }
    if (ABLV == 2) HIP_TRY(launch(kern_c<bwd_own_d16_kernel<false, OWN_NW, OWN_K, 2>>));
    else if (ABLV == 8) HIP_TRY(launch(kern_c<bwd_own_d16_kernel<false, OWN_NW, OWN_K, 8>>));
    else if (ABLV == 16) HIP_TRY(launch(kern_c<bwd_own_d16_kernel<false, OWN_NW, OWN_K, 16>>));
    else HIP_TRY(launch(kern_c<bwd_own_d16_kernel<false, OWN_NW, OWN_K, 0>>));
    return RGCN_OK;
  }
#endif
  if (packed && (flags & RGCN_F_RELU)) HIP_TRY(launch(kern_c<bwd_own_d16_kernel<true, OWN_NW, OWN_K, 0, false, true>>));
  else if (packed) HIP_TRY(launch(kern_c<bwd_own_d16_kernel<false, OWN_NW, OWN_K, 0, false, true>>));
  else if (flags & RGCN_F_RELU) HIP_TRY(launch(kern_c<bwd_own_d16_kernel<true, OWN_NW, OWN_K>>));
  else HIP_TRY(launch(kern_c<bwd_own_d16_kernel<false, OWN_NW, OWN_K>>));
  return RGCN_OK;
}

extern "C" int rgcn_bwd_own_bf16(const uint16_t *G, const uint16_t *X, const float *Wt_packed, uint16_t *dX, float *dW, const void *rec,
                                 const int32_t *own_ptr, const int32_t *group_ptr, int32_t shared_rel, const int32_t *unit_rel, int64_t n_tiles,
                                 int32_t tile_rows, int64_t n_dst, int32_t R, int32_t flags, float *dbias, int64_t n_src, void *stream) {
  if (!G || !X || !Wt_packed || !dX || !dW || !rec || !unit_rel || n_tiles <= 0 || tile_rows <= 0 || n_dst <= 0 || R <= 0 ||
      R > 0xFFFF || n_dst > INT32_MAX || n_tiles * (int64_t)OWN_NW >= INT32_MAX || n_src <= 0 || n_src >= (int64_t(1) << 26) || (flags & ~RGCN_F_PACKED_REC) != 0 ||
      !own_groups_ok(own_ptr, group_ptr, shared_rel, n_tiles, R)) {
    rgcn_set_error("bwd_own_bf16: bad argument (the records address G rows as src << 6 in 32 bits: n_src < 2^26; no flags)");
    return RGCN_EINVAL;
  }
  const bool packed = (flags & RGCN_F_PACKED_REC) != 0;
  if (tile_rows > (packed ? OWN_MAX_ROWS_PK : OWN_MAX_ROWS)) {
    rgcn_set_error("bwd_own_bf16: tiles of at most %d rows (got %d)", packed ? OWN_MAX_ROWS_PK : OWN_MAX_ROWS, tile_rows);
    return RGCN_EUNSUPPORTED;
  }
  hipStream_t st = (hipStream_t)stream;
  int dev = 0, n_cu = 0;
  HIP_TRY(launch_device(&dev, &n_cu));
  HIP_TRY(zero_dw_dbias_async(dW, (size_t)R, dbias, st));
  const size_t lds = bwd_own_lds(tile_rows, packed);
  const unsigned n_blocks = (unsigned)std::min<int64_t>(n_tiles, n_cu);
  auto launch = [&](auto k) -> hipError_t {
    constexpr auto kern = decltype(k)::value;
    hipError_t e = allow_lds<kern>(dev, lds, OWN_LDS_MAX);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, dim3(n_blocks), dim3(64 * OWN_NW), lds, st, reinterpret_cast<const float *>(G), reinterpret_cast<const float *>(X),
                       Wt_packed, reinterpret_cast<float *>(dX), dW, static_cast<const char *>(rec), group_ptr ? group_ptr : own_ptr,
                       group_ptr ? OWN_NW + 1 : OWN_NW, group_ptr ? shared_rel : -1, (int)n_tiles, tile_rows, (int)n_dst, dbias, (int)n_src, unit_rel);
    return hipGetLastError();
  };
  if (packed) HIP_TRY(launch(kern_c<bwd_own_d16_kernel<false, OWN_NW, OWN_K, 0, true, true>>));
  else HIP_TRY(launch(kern_c<bwd_own_d16_kernel<false, OWN_NW, OWN_K, 0, true>>));
  return RGCN_OK;
}
