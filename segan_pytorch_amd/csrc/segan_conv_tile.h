// Device-side pieces of a contraction tile shared by the fp32 kernels (segan_conv.hip), the bf16 /
// bf16x3 kernel (segan_conv_bf2.hip) and the weight gradients: tile geometry, per-lane column
// bookkeeping, the stream-K accumulator slabs, THE tile epilogue and the stream-K fix-up kernel.
#pragma once
#include "segan_conv_shared.h"

// Tile geometry: MB rows x NB columns per 256-thread workgroup, waves WM x (4/WM).
//   F form: rows = output channels m; waves 2x2.
//   T form: rows = (phase r, channel n) with ALL S phases of MB/S channels in one tile and
//           waves 1x4 (NB=128) so that one lane ends up holding the S consecutive output
//           samples S*q..S*q+S-1 of a channel: full-line stores instead of stride-S ones.
template <int MB, int NB, int WM, int U>
struct TileGeom {
  static constexpr int S = 32 / U;
  static constexpr int WN = 4 / WM;
  static constexpr int NI = MB / (32 * WM);
  static constexpr int NJ = NB / (32 * WN);
  static constexpr int NPT = MB / S;   // T form: channels per tile
};

// per-lane column bookkeeping of a tile: which (sample, time) the lane's NJ columns are and
// where they sit in the LDS activation tile
template <int NB, int WN, int NJ>
__device__ __forceinline__ void lane_columns(const CorrArgs& a, const ColTile& ct, int wn, int l31,
                                             int h, int (&col_b)[NJ], int (&col_t)[NJ],
                                             int (&boff)[NJ]) {
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int cl = wn * (NB / WN) + 32 * j + l31;
    const int col = ct.col0 + cl;
    if (col < a.Ctot) {
      const int b = col / a.Tcols;
      col_b[j] = b;
      col_t[j] = col - b * a.Tcols;
      boff[j] = cl + (b - ct.b0) * a.H + h;
    } else {
      col_b[j] = -1;
      col_t[j] = 0;
      boff[j] = h;
    }
  }
}

// accumulator slab of a stream-K piece (and of a contraction split of the deterministic weight
// gradients): [NI*NJ*4][256] float4, thread-minor (coalesced 16-byte accesses)
template <int NI, int NJ>
__device__ __forceinline__ void slab_store(float* slab, const f32x16 (&acc)[NI][NJ], int tid) {
  f32x4* s4 = reinterpret_cast<f32x4*>(slab);
#pragma unroll
  for (int i = 0; i < NI; ++i)
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const f32x4 v = {acc[i][j][4 * q], acc[i][j][4 * q + 1], acc[i][j][4 * q + 2],
                         acc[i][j][4 * q + 3]};
        s4[((i * NJ + j) * 4 + q) * 256 + tid] = v;
      }
}
template <int NI, int NJ>
__device__ __forceinline__ void slab_add(const float* slab, f32x16 (&acc)[NI][NJ], int tid) {
  const f32x4* s4 = reinterpret_cast<const f32x4*>(slab);
#pragma unroll
  for (int i = 0; i < NI; ++i)
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const f32x4 v = s4[((i * NJ + j) * 4 + q) * 256 + tid];
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[i][j][4 * q + e] += v[e];
      }
}

// ---- epilogue: bias, optional tanh, store of a finished tile ----
// One copy for every contraction kernel and for the stream-K fix-up.  The generic per-element forms
// (64-bit address arithmetic, row / destination tests and a bias load per element) spend ~30 VALU per
// stored value: a tenth of a 64-chunk fp32 tile's time, and — a bf16 tile spends 16x fewer
// matrix-pipe cycles per output element — as much as a bf16 tile's whole contraction.  Tiles whose
// rows are all real channels of one destination therefore take fast forms whose per-lane byte offsets
// are computed once per COLUMN (masked columns carry an out-of-range offset: the store is dropped).
//
// PAIR_OK: whether the stride-2 pair stores below are compiled in.  On for the fp32 kernels.  Off
// for the bf16 ones: with them the stride-2 T instantiations of corr_bf2_kernel spill (bf16: 144 ->
// 168 VGPRs, 21 of them spilled, 88 B/lane of scratch; bf16x3: 163 -> 210 VGPRs, 3 -> 2 waves per
// SIMD; kernel-resource-usage remarks), so those keep the per-element form for stride 2.
template <int MB, int NB, int WM, int U, bool OUT_HI, bool PAIR_OK>
__device__ __forceinline__ void corr_store_tile(
    const CorrArgs& a, const f32x16 (&acc)[TileGeom<MB, NB, WM, U>::NI][TileGeom<MB, NB, WM, U>::NJ],
    int m0, int n0, int wm, int h, const int (&col_b)[TileGeom<MB, NB, WM, U>::NJ],
    const int (&col_t)[TileGeom<MB, NB, WM, U>::NJ]) {
  using G = TileGeom<MB, NB, WM, U>;
  constexpr int S = G::S, NI = G::NI, NJ = G::NJ, NPT = G::NPT;
  if (!OUT_HI) {
    // Interior tiles — all rows valid and in one destination, plain stores — take the fast form:
    // buffer stores with the per-column offsets, the row inside the tile goes through the scalar
    // offset: no address arithmetic, row test or destination select per element.
    {
      float* fdst = m0 < a.OC0 ? a.out0 : a.out1;
      const int foc = m0 < a.OC0 ? a.OC0 : a.OC1;
      const int foch = m0 < a.OC0 ? m0 : m0 - a.OC0;
      const long fbytes = (long)a.B * foc * a.Lout * 4;
      if (a.act == SEGAN_ACT_NONE && m0 + MB <= a.Rvalid && (m0 + MB <= a.OC0 || m0 >= a.OC0) &&
          fdst != nullptr && fbytes < 0x7fffffffL) {
        const __amdgpu_buffer_rsrc_t ors =
            __builtin_amdgcn_make_buffer_rsrc(fdst, 0, (int)fbytes, 0x00020000);
        int ovo[NJ];
#pragma unroll
        for (int j = 0; j < NJ; ++j)
          ovo[j] = col_b[j] < 0 ? (int)0x80000000u
                                : ((col_b[j] * foc + foch + 32 * wm * NI + 4 * h) * a.Lout + col_t[j]) * 4;
        const int rowstep = a.Lout * 4;
#pragma unroll
        for (int i = 0; i < NI; ++i) {
#pragma unroll
          for (int e = 0; e < 16; ++e) {
            const int rl = 32 * i + (e & 3) + 8 * (e >> 2);
            float bs = 0.0f;
            if (a.bias) bs = epi_bias(a.bias, m0 + 32 * wm * NI, rl, h);
#pragma unroll
            for (int j = 0; j < NJ; ++j)
              __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, acc[i][j][e] + bs), ors,
                                                    ovo[j], rl * rowstep, 0);
          }
        }
        return;
      }
    }
#pragma unroll
    for (int i = 0; i < NI; ++i) {
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int row = m0 + 32 * (wm * NI + i) + (e & 3) + 8 * (e >> 2) + 4 * h;
        if (row >= a.Rvalid) continue;
        // LO store: out[b, row, t]
        float* dst;
        int oc, och;
        if (row < a.OC0) { dst = a.out0; oc = a.OC0; och = row; }
        else { dst = a.out1; oc = a.OC1; och = row - a.OC0; }
        if (dst == nullptr) continue;
        const float bs = a.bias ? a.bias[row] : 0.0f;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
          if (col_b[j] < 0) continue;
          float v = acc[i][j][e] + bs;
          if (a.act == SEGAN_ACT_TANH) v = tanhf(v);
          dst[((size_t)col_b[j] * oc + och) * (size_t)a.Lout + col_t[j]] = v;
        }
      }
    }
  } else {
    // HI store.  Row block ib of the tile is phase r = 32*ib / NPT of channels n0 + nl.
    constexpr bool QUAD = (S == 4 && WM == 1 && NI == 4);  // lane holds all 4 phases of (n, q)
    const int hl = a.o_padL + a.o_padR;
    const long obytes = (long)a.B * a.Nout * a.Lout * 4;
    const bool qfast = obytes < 0x7fffffffL;      // 32-bit byte offsets reach every output element
    const __amdgpu_buffer_rsrc_t qrs = __builtin_amdgcn_make_buffer_rsrc(
        a.out0, 0, (int)(qfast ? obytes : 0), 0x00020000);
    if (QUAD && qfast && a.act == SEGAN_ACT_NONE && a.o_padL == 0 && a.o_roll == 0 &&
        a.halo == nullptr && n0 + NPT <= a.Nout && a.Lout == 4 * a.Tcols) {
      // deconv forward: a lane's four phase accumulators are four consecutive output samples
      int ovo[NJ];
#pragma unroll
      for (int j = 0; j < NJ; ++j)
        ovo[j] = col_b[j] < 0 ? (int)0x80000000u
                              : ((col_b[j] * a.Nout + n0 + 4 * h) * a.Lout + 4 * col_t[j]) * 4;
      const int rowstep = a.Lout * 4;
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int nl = (e & 3) + 8 * (e >> 2);
        float bs = 0.0f;
        if (a.bias) bs = epi_bias(a.bias, n0, nl, h);
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
          typedef unsigned u32x4s __attribute__((ext_vector_type(4)));
          const u32x4s o = {__builtin_bit_cast(unsigned, acc[0 % NI][j][e] + bs),
                            __builtin_bit_cast(unsigned, acc[1 % NI][j][e] + bs),
                            __builtin_bit_cast(unsigned, acc[2 % NI][j][e] + bs),
                            __builtin_bit_cast(unsigned, acc[3 % NI][j][e] + bs)};
          __builtin_amdgcn_raw_buffer_store_b128(o, qrs, ovo[j] + nl * rowstep, 0, 0);   // (*)
        }
      }
      return;
    }
    int cb[NJ];          // columns still to be stored by the generic form below (-1: done / masked)
#pragma unroll
    for (int j = 0; j < NJ; ++j) cb[j] = col_b[j];
    if (QUAD && qfast && a.act == SEGAN_ACT_NONE && n0 + NPT <= a.Nout) {
      // conv data gradient (HI store with a left pad, a halo and possibly a roll): everything that
      // depends on the COLUMN only — sample, the first of the lane's four output positions, the
      // roll's wrap — is worked out once per column instead of once per stored vector; interior
      // columns (all but the ~8 at a row's ends and the one on the wrap point) then store one
      // 16-byte vector per channel row (the row offset added to the vector offset: (*) in
      // segan_conv_shared.h).  The generic form below costs a bf16 tile 40 % of its time (measured
      // with the stores compiled out, on enc1 / enc2's data gradients) and an fp32 tile
      // 5-10 %.
      int ovo[NJ];
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        ovo[j] = (int)0x80000000u;
        if (col_b[j] >= 0) {
          const int i0 = 4 * col_t[j] - a.o_padL;
          int ib = i0 - a.o_roll;
          if (ib < 0) ib += a.Lout;
          if (ib >= a.Lout) ib -= a.Lout;
          if (i0 >= 0 && i0 + 3 < a.Lout && ib + 3 < a.Lout) {
            ovo[j] = ((col_b[j] * a.Nout + n0 + 4 * h) * a.Lout + ib) * 4;
            cb[j] = -1;
          }
        }
      }
      const int rowstep = a.Lout * 4;
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int nl = (e & 3) + 8 * (e >> 2);
        float bs = 0.0f;
        if (a.bias) bs = epi_bias(a.bias, n0, nl, h);
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
          typedef unsigned u32x4s __attribute__((ext_vector_type(4)));
          const u32x4s o = {__builtin_bit_cast(unsigned, acc[0 % NI][j][e] + bs),
                            __builtin_bit_cast(unsigned, acc[1 % NI][j][e] + bs),
                            __builtin_bit_cast(unsigned, acc[2 % NI][j][e] + bs),
                            __builtin_bit_cast(unsigned, acc[3 % NI][j][e] + bs)};
          __builtin_amdgcn_raw_buffer_store_b128(o, qrs, ovo[j] + nl * rowstep, 0, 0);   // (*)
        }
      }
      bool left = false;
#pragma unroll
      for (int j = 0; j < NJ; ++j) left = left || cb[j] >= 0;
      if (!left) return;
    }
    // Stride 2: a lane holds BOTH phases of its channels — in row blocks ib and ib + NI/2
    // (64 / 32 channels per tile), or in elements e and e + 8 of the one block of a 16-channel tile —
    // i.e. two consecutive output samples: one 8-byte store per (channel, column) for the deconv
    // forward and the interior columns of the conv data gradient, offsets once per column as in the
    // stride-4 form above.  The stride-2 T form used to take the generic per-element path below.
    constexpr bool PAIR = PAIR_OK && (S == 2 && WM == 1 && (NI == 4 || NI == 2 || NI == 1));
    if (PAIR && qfast && a.act == SEGAN_ACT_NONE && n0 + NPT <= a.Nout) {
      int ovo[NJ];
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        ovo[j] = (int)0x80000000u;
        if (col_b[j] >= 0) {
          const int i0 = 2 * col_t[j] - a.o_padL;
          int ib = i0 - a.o_roll;
          if (ib < 0) ib += a.Lout;
          if (ib >= a.Lout) ib -= a.Lout;
          if (i0 >= 0 && i0 + 1 < a.Lout && ib + 1 < a.Lout) {
            ovo[j] = ((col_b[j] * a.Nout + n0 + 4 * h) * a.Lout + ib) * 4;
            cb[j] = -1;
          }
        }
      }
      const int rowstep = a.Lout * 4;
      constexpr int NBLK = NI >= 2 ? NI / 2 : 1;      // 32-channel blocks of the tile
      constexpr int NE = NI >= 2 ? 16 : 8;            // channel slots per block and lane
#pragma unroll
      for (int bk = 0; bk < NBLK; ++bk) {
#pragma unroll
        for (int e = 0; e < NE; ++e) {
          const int nl = 32 * bk + (e & 3) + 8 * (e >> 2);
          float bs = 0.0f;
          if (a.bias) bs = epi_bias(a.bias, n0, nl, h);
#pragma unroll
          for (int j = 0; j < NJ; ++j) {
            typedef unsigned u32x2s __attribute__((ext_vector_type(2)));
            const float p0 = acc[bk][j][e];
            const float p1 = NI >= 2 ? acc[(bk + NI / 2) % NI][j][e] : acc[0][j][(e + 8) % 16];
            const u32x2s o = {__builtin_bit_cast(unsigned, p0 + bs), __builtin_bit_cast(unsigned, p1 + bs)};
            __builtin_amdgcn_raw_buffer_store_b64(o, qrs, ovo[j] + nl * rowstep, 0, 0);   // (*)
          }
        }
      }
      bool left = false;
#pragma unroll
      for (int j = 0; j < NJ; ++j) left = left || cb[j] >= 0;
      if (!left) return;
    }
#pragma unroll
    for (int e = 0; e < 16; ++e) {
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        if (cb[j] < 0) continue;
        const int q = col_t[j];
        if (QUAD) {
          const int n = n0 + (e & 3) + 8 * (e >> 2) + 4 * h;
          if (n >= a.Nout) continue;
          const float bs = a.bias ? a.bias[n] : 0.0f;
          float v[4];
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            v[r] = acc[r][j][e] + bs;
            if (a.act == SEGAN_ACT_TANH) v[r] = tanhf(v[r]);
          }
          const size_t rowoff = (size_t)col_b[j] * a.Nout + n;
          const int i0 = 4 * q - a.o_padL;
          if (qfast && i0 >= 0 && i0 + 3 < a.Lout) {
            // interior of the row (all but ~8 of its positions): the four phases are four
            // consecutive samples, also after the roll unless they straddle its wrap point
            int ib = i0 - a.o_roll;
            if (ib < 0) ib += a.Lout;
            if (ib >= a.Lout) ib -= a.Lout;
            if (ib + 3 < a.Lout) {
              typedef unsigned u32x4s __attribute__((ext_vector_type(4)));
              const u32x4s o = {__builtin_bit_cast(unsigned, v[0]), __builtin_bit_cast(unsigned, v[1]),
                                __builtin_bit_cast(unsigned, v[2]), __builtin_bit_cast(unsigned, v[3])};
              __builtin_amdgcn_raw_buffer_store_b128(o, qrs, (int)((rowoff * a.Lout + ib) * 4), 0, 0);
              continue;
            }
          }
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int P = 4 * q + r;
            int ii = P - a.o_padL;
            if (ii >= 0 && ii < a.Lout) {
              if (a.o_roll != 0) {
                ii -= a.o_roll;
                if (ii < 0) ii += a.Lout;
                if (ii >= a.Lout) ii -= a.Lout;
              }
              a.out0[rowoff * (size_t)a.Lout + ii] = v[r];
            } else if (a.halo != nullptr) {
              if (ii < 0) a.halo[rowoff * hl + P] = v[r];
              else if (ii - a.Lout < a.o_padR) a.halo[rowoff * hl + a.o_padL + (ii - a.Lout)] = v[r];
            }
          }
        } else {
#pragma unroll
          for (int i = 0; i < NI; ++i) {
            const int rloc = 32 * (wm * NI + i) + (e & 3) + 8 * (e >> 2) + 4 * h;
            const int r = rloc / NPT;
            const int n = n0 + rloc % NPT;
            if (n >= a.Nout) continue;
            float v = acc[i][j][e] + (a.bias ? a.bias[n] : 0.0f);
            if (a.act == SEGAN_ACT_TANH) v = tanhf(v);
            const int P = S * q + r;
            int ii = P - a.o_padL;
            const size_t rowoff = (size_t)col_b[j] * a.Nout + n;
            if (ii >= 0 && ii < a.Lout) {
              if (a.o_roll != 0) {
                ii -= a.o_roll;
                if (ii < 0) ii += a.Lout;
                if (ii >= a.Lout) ii -= a.Lout;
              }
              a.out0[rowoff * (size_t)a.Lout + ii] = v;
            } else if (a.halo != nullptr) {
              if (ii < 0) a.halo[rowoff * hl + P] = v;
              else if (ii - a.Lout < a.o_padR) a.halo[rowoff * hl + a.o_padL + (ii - a.Lout)] = v;
            }
          }
        }
      }
    }
  }
}

// F form: rows of a tile that all go to a NULL destination (the z half of the first decoder
// layer's data gradient) are skipped
template <int MB, bool OUT_HI>
__device__ __forceinline__ bool tile_is_dead(const CorrArgs& a, int m0) {
  if (OUT_HI) return false;
  if (a.out0 == nullptr && m0 + MB <= a.OC0) return true;
  if (a.out1 == nullptr && m0 >= a.OC0) return true;
  return false;
}

// Stream-K second pass: one workgroup per cut tile of `nch` chunks (fp32) or weight stages (bf16)
// adds the slabs of its pieces in chunk order — a fixed order, no atomics, no zero-filled outputs:
// results are bit-reproducible — and stores the tile.  Tiles that one workgroup happened to hold
// whole were stored by the main kernel.
// FLY: slabs loaded before they are added.  The kernel is a pure stream, and 2 keeps more loads
// outstanding per lane (the fp32 launchers), at 200 VGPRs for a 128 x 128 tile: 2 workgroups of a
// SIMD's 4 slots.  The bf16 launches cut up to three rounds' worth of tiles (568 of enc3's data
// gradient at B = 300) and keep 1: 88 - 104 VGPRs, 4 - 5 resident — with 2 that layer measured 5 %
// slower (profiles/epilogue_share_ab.json).
template <int MB, int NB, int WM, int U, bool OUT_HI, bool PAIR_OK, int FLY>
__global__ __launch_bounds__(256) void corr_fixup_kernel(const CorrArgs a, int nch) {
  using G = TileGeom<MB, NB, WM, U>;
  constexpr int WN = G::WN, NI = G::NI, NJ = G::NJ, NPT = G::NPT;
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // uniform: scalar bias loads (epi_bias)
  const int wm = wave / WN, wn = wave % WN;
  const int l31 = lane & 31, h = lane >> 5;
  const int t = blockIdx.x;
  const long u0 = (long)t * nch, u1 = u0 + nch - 1;
  const int g_first = (int)(u0 / a.sk_units), g_last = (int)(u1 / a.sk_units);
  if (g_first == g_last) return;
  // tile -> (row tile, column tile): rows first (a.tile_order, bf16 only) or columns first
  const int tile = a.sk_nfull + t;
  const int coltile = a.tile_order ? tile / a.nrt : tile % a.ncoltiles;
  const int rowtile = a.rt0 + (a.tile_order ? tile - coltile * a.nrt : tile / a.ncoltiles);
  const int m0 = rowtile * MB, n0 = rowtile * NPT;
  if (tile_is_dead<MB, OUT_HI>(a, m0)) return;
  const ColTile ct = make_coltile(coltile * NB, a.Tcols, NB);
  int col_b[NJ], col_t[NJ], boff[NJ];
  lane_columns<NB, WN, NJ>(a, ct, wn, l31, h, col_b, col_t, boff);
  f32x16 acc[NI][NJ];
#pragma unroll
  for (int i = 0; i < NI; ++i)
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.0f;
  // FLY pieces in flight at a time, always ADDED in chunk order
  constexpr int NV = NI * NJ * 4;
  for (int g = g_first; g <= g_last; g += FLY) {
    f32x4 v[FLY][NV];
#pragma unroll
    for (int f = 0; f < FLY; ++f) {
      if (g + f > g_last) break;
      const int piece = t - (int)(((long)(g + f) * a.sk_units) / nch);
      const f32x4* s4 = reinterpret_cast<const f32x4*>(a.sk_ws + (size_t)((g + f) * 2 + piece) * (MB * NB));
#pragma unroll
      for (int q = 0; q < NV; ++q) v[f][q] = s4[q * 256 + tid];
    }
#pragma unroll
    for (int f = 0; f < FLY; ++f) {
      if (g + f > g_last) break;
#pragma unroll
      for (int q = 0; q < NV; ++q)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[q / (NJ * 4)][(q / 4) % NJ][4 * (q % 4) + e] += v[f][q][e];
    }
  }
  corr_store_tile<MB, NB, WM, U, OUT_HI, PAIR_OK>(a, acc, m0, n0, wm, h, col_b, col_t);
}
