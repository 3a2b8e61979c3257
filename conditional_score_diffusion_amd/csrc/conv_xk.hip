// conv_xk.hip - the fp16x3 (fp32-class) fused-prologue 3x3 convolution of the 160^2 / 80^2 / 40^2 levels
// (reference models/layers.py:119-132,632-675: h = Conv(act(GroupNorm(x))) [+ Dense(temb)] / x + Conv(...); models/layerspp.py:212-274)
// in the 1-D Winograd F(2,3) form along the image row, one transform component per wave.
//
// Arithmetic.  For an output pair (y0, y1) of a row, inputs d0..d3 and a filter row (g0, g1, g2):
//     D0 = d0 - d2   D1 = d1 + d2   D2 = d2 - d1   D3 = d1 - d3                       (input transform, fp32, BEFORE the hi | lo split)
//     G0 = g0        G1 = (g0 + g1 + g2) / 2       G2 = (g0 - g1 + g2) / 2   G3 = g2  (weights, transformed at pack time)
//     Mk = sum over input channels and the 3 filter ROWS of Dk * Gk                   (4 contractions instead of 6 per output pair)
//     y0 = M0 + M1 + M2      y1 = M1 - M2 - M3                                        (output transform in the epilogue)
// Every operand is carried as hi + lo fp16 (22 significand bits), products lo * hi, hi * hi, hi * lo on v_mfma_f32_32x32x16_f16 with fp32
// accumulation: 2 MFMAs per algorithmic product (the direct form: 3).  A 16-channel stage of a 16 x 16-pixel x 32 NT-cout tile is 3 row
// taps x 12 NT MFMAs.  Packed weights: [cout group][cin / 16][filter row][component][cout tile][hi | lo][64 lanes x 8 halves], x 2^8.
//
// Structure (the lineage conv_xp -> conv_xw -> conv_xk is in profiles/NOTEBOOK.md, rounds 4 - 5; the two predecessors were removed from
// the tree in round 6): ONE persistent 4-wave workgroup per CU (512 registers per lane), every wave ONE instruction stream
//     MFMA | 2 - 5 "filler" instructions | MFMA | ...
// with the fillers pinned in program order by scheduling fences - what hides behind a matrix instruction is the SAME wave's next few
// instructions (MI355X_MICROARCH.md: ~5 single-issue instructions per 32-cycle MFMA gap with one wave per SIMD).  The fillers are the
// conversion of the NEXT stage's operand patch (GroupNorm affine + exp2-domain SiLU + input transform + hi | lo split, on UNITS of two
// adjacent patch pixels x 4 channels with the right-hand neighbour's values by ds_bpermute; the float4s were requested two stages
// earlier), the ds_read_b128 of the next row tap's fragments, the weight requests and, in a tile's last stage, the epilogue's requests.
// The matrix instructions are asm statements (hipcc kept accumulators in VGPRs across joins and copied them through v_accvgpr_*; an asm
// MFMA is opaque to its hazard tracker, so the epilogue's reads sit behind a tied wait and tools/check_xp_isa.py checks every build).
//
// Ownership: WAVE k OWNS TRANSFORM COMPONENT k for all 128 pixel pairs of the tile (4 M tiles x NT cout tiles = 4 NT accumulators).  A wave
// then needs only its own component's weights: 2 NT KiB per row tap, straight from L2 into registers (three register sets, one per row
// tap, each refilled two row taps before its next use) - no weight staging through LDS (in the predecessor, where every wave multiplied
// all four components: 72 ds_write_b128 per stage into a three-slot ring and a workgroup barrier per row tap, 1.0 k of a stage's 6.05 k
// cycles for the stores alone), ONE barrier per stage (the patch double buffer; in front of the stage's last row tap, whose fragments are
// already in registers), 8 instead of 32 fragment reads per row tap.  The price is paid once per tile: the output transform needs the four
// components of a pixel pair in ONE lane, so the epilogue turns them through LDS - per row of a wave's 4 x 16-pixel block every wave
// stores its component of all four blocks (12 ds_write_b128 straight from the accumulator registers), one barrier, 12 ds_read_b128 of
// the four components of its own block; the rounds alternate between two LDS regions (the dead patch buffer + the space between the
// patch buffers | the top of LDS).
// Product order per row tap: lo * hi, hi * hi, hi * lo (the lo pixel fragments are free after the first product, the hi ones M tile by
// M tile under the last: both are re-read for the NEXT row tap inside the current one, so no fragment of a stage's patch is read after
// the barrier in front of its last row tap).
//
// Tile height.  A tile is 4 MT rows x 16 columns, MT = 4 everywhere but in the bottom tile row of a map with H % 16 == 8 (the 40^2 level
// of the 160^2 networks: 40 = 16 + 16 + 8), whose tiles are 8 rows high: MT = 2 - 2 NT accumulators and 6 NT MFMAs per row tap, a patch
// of 10 rows (90 conversion units on two request / conversion slots), exchange stores for blocks 0 and 1 only.  Per accumulator the
// MFMA order, in the epilogue the block ownership (wave w owns block w; waves 2 and 3 send, meet the barriers and contribute exact
// zeros to the statistics, as their masked lanes did on a 16-row tile), the statistics chains and the tile's slot of the fp64 partials
// are those of the 16-row tile: results are bit-identical to running the bottom row on 16-row tiles.  Such a layer is ONE launch that
// holds both walks; a workgroup walks tiles of one height only (conv_xk_kernel below, the split of the grid in launch_xk).  Half the
// MFMA gaps per stage carry two thirds of the conversion (two slots of three), so the MT = 2 stage is the denser one: its operations
// are spread over the gaps of all three row taps (conv_xk_walk.inc, "MT = 2"), where the MT = 4 stage spreads each tap's own.
#include "conv_ff.h"

#include <utility>

namespace csd {

#define XW_THREADS 256
#define XW_RS (32 * 64 + 16)                         // LDS pitch of a transformed patch row: (component, pair) records of 64 B (16 ch hi | 16 ch lo)
#define XW_PATCH_BYTES (FF_PW * XW_RS)               // 37152

template <int NT_, int MT_ = 4>
struct XKCfg {
  static constexpr int NT = NT_, MT = MT_;                   // cout tiles | M tiles (4 rows x 16 columns each) of a tile: 4 = 16 rows, 2 = 8 rows
  static constexpr int NA = MT * NT;                         // accumulators per wave = MFMAs per product
  static constexpr int NSLOT = MT == 4 ? 3 : 2;              // request / conversion slots per stage (60 units each)
  static constexpr int NU = 9 * (4 * MT + 2);                // conversion units per stage: 4 MT + 2 patch rows x 9 column pairs (162 | 90)
  static constexpr int GP = 3 * NA;                          // MFMAs (= filler gaps) per row tap
  static constexpr int TAPB = 4 * NT * 2 * 1024;             // weight bytes per row tap: 4 components x NT cout tiles x (hi | lo)
  static constexpr int STB = 3 * TAPB;                       // per stage
  static constexpr int WPT = 2 * NT;                         // 1 KiB pieces per wave and row tap
  // LDS map (XTOG = the distance of the two patch buffers: a toggle is one xor): [0, 37152) patch 0 | exchange region X, blocks 2 and 3 | dummy | [65536, 102688) patch 1 |
  // exchange region Y, slots 0 .. 7 | the dummy's partner | [131072, ..) region Y, slots 8 .. 15 | red.  Region X's blocks 0 and 1 take
  // the patch buffer that is dead during the epilogue.  A slot = (destination block, source component): NT KiB.
  static constexpr int XTOG = 65536;
  static constexpr int SLOTB = NT * 1024;
  static constexpr int OFF_X23 = XW_PATCH_BYTES, OFF_DUMMY = OFF_X23 + 8 * SLOTB, OFF_Y0 = XTOG + XW_PATCH_BYTES, OFF_Y8 = 2 * XTOG;
  static constexpr int OFF_RED = OFF_Y8 + 8 * SLOTB;
  static constexpr size_t LDS = (size_t)OFF_RED + 4 * NT * 32 * 2 * sizeof(float);
  static_assert(OFF_DUMMY + 3072 <= XTOG && OFF_Y0 + 8 * SLOTB <= OFF_DUMMY + XTOG && OFF_DUMMY + XTOG + 3072 <= OFF_Y8 && 8 * SLOTB <= XW_PATCH_BYTES &&
                    LDS <= 160 * 1024,
                "conv_xk: LDS map");
};

template <class F, int... I>
__device__ __forceinline__ void xk_static_for_impl(F&& f, std::integer_sequence<int, I...>) {
  (f(std::integral_constant<int, I>{}), ...);
}
template <int N, class F>
__device__ __forceinline__ void xk_static_for(F&& f) {
  xk_static_for_impl(static_cast<F&&>(f), std::make_integer_sequence<int, N>{});
}

typedef unsigned int xk_u4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ int xk_pack_f16(float a, float b) {
  typedef float f2 __attribute__((ext_vector_type(2)));
  typedef _Float16 h2 __attribute__((ext_vector_type(2)));
  return __builtin_bit_cast(int, __builtin_convertvector(f2{a, b}, h2));
}
template <bool HIGH>
__device__ __forceinline__ float xk_lo(int hp, float v) {      // v - (float)half: one v_fma_mix_f32 (exact)
  float r;
  if constexpr (HIGH) asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(r) : "v"(hp), "v"(v));
  else asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel_hi:[1,0,0]" : "=v"(r) : "v"(hp), "v"(v));
  return r;
}

#define XW_FENCE() __builtin_amdgcn_sched_barrier(0)
#define XW_SADD(x, y) asm volatile("s_add_u32 %0, %0, %1" : "+s"(x) : "s"(y) : "scc")
#define XW_PIN(a) asm volatile("" : "+v"(a))
// tuning aids (never in the product library): XK_ABL bits remove parts of the stream at compile time (results are then garbage):
// 1 conversion, 2 weight requests, 4 fragment reads, 8 output stores, 16 patch requests, 32 residual requests, 64 the stage barriers,
// 128 the epilogue's exchange stores, 65536 its barriers, 131072 its reads (own accumulators instead), 262144 its statistics,
// 524288 the whole row loop of the epilogue (what remains is the tile switch),
// 256 patch stores, 512 neighbour exchange (own value instead), 1024 transcendentals (plain multiplies instead), 2048 hi | lo split,
// 4096 patch requests confined to the first 256 pixels of the sample (cache hits), 8192 the same bytes as whole 1 KiB pieces
// (tools/xk_abl_build.sh builds the libraries, tools/xk_timing.py reads the per-tile stamps)
#ifndef XK_ABL
#define XK_ABL 0
#endif
// Tuning-build stamps sit at TILE boundaries only (the loop top: no accumulator is live there).  A stamp is a branch; between a tile's
// first MFMA and its epilogue's last accumulator read a control-flow edge lets hipcc move accumulators - unprotected reads of matrix
// results: per-unit stamps made the tuning build return NaN, and tools/check_xp_isa.py now checks the tuning build as well.
#ifdef CSD_FF_TUNE
#define XW_WALL(i) do { if (a_dbg && tid == 0) a_dbg[blockIdx.x * 32 + (i)] = wall_clock64(); } while (0)
#else
#define XW_WALL(i) do { } while (0)
#endif

// ---- the filler schedule of a row tap (compile time) ----
// MFMA g of a row tap: product g / PB (0 lo * hi, 1 hi * hi, 2 hi * lo), M tile (g % PB) / NT, cout tile g % NT.  Fixed fillers of gap g:
template <int NT, int MT = 4>
struct XKSched {
  static constexpr int PB = MT * NT, GP = 3 * PB, WPT = 2 * NT;
  static constexpr bool rd_xl(int g) { return g < PB && g % NT == NT - 1; }                          // xl[g / NT] of the NEXT tap (its last use was MFMA g)
  static constexpr bool rd_xh(int g) { return g >= 2 * PB && g % NT == NT - 1; }                     // xh[(g - 2 PB) / NT] of the next tap
  static constexpr bool slot_req(int g) { return g == 0; }                                           // the tap's two patch requests
  static constexpr bool ld_w(int g) { return g >= PB && g < PB + WPT; }                              // weight fragment g - PB of the tap two ahead
  static constexpr int fixed(int g) { return (rd_xl(g) ? 1 : 0) + (rd_xh(g) ? 1 : 0) + (ld_w(g) ? 1 : 0) + (slot_req(g) ? 3 : 0); }
  static constexpr int wgt(int g) { return 14 - 3 * fixed(g) > 2 ? 14 - 3 * fixed(g) : 2; }
  static constexpr int cum(int g) { int s = 0; for (int h = 0; h < g; ++h) s += wgt(h); return s; }
  static constexpr int first_op(int n, int g) { return (int)(((long long)n * cum(g)) / cum(GP)); }    // ops [first_op(n, g), first_op(n, g + 1)) in gap g
  // the same over the gaps of all three row taps of a stage (the half-height walk: one operation sequence per stage)
  static constexpr int first_op3(int n, int r, int g) { return (int)(((long long)n * (r * cum(GP) + cum(g))) / (3 * cum(GP))); }
};

#define XK_MFMA_AV(ACC, A, B) asm volatile("v_mfma_f32_32x32x16_f16 %0, %1, %2, %0" : "+a"(ACC) : "a"(A), "v"(B))
#define XK_MFMA_AA(ACC, A, B) asm volatile("v_mfma_f32_32x32x16_f16 %0, %1, %2, %0" : "+a"(ACC) : "a"(A), "a"(B))

// The kernel's body - one workgroup's walk over its tiles of 4 MT rows x 16 columns - is conv_xk_walk.inc, included once per walk
// (XK_WALK_MT: the M tiles of a tile; XK_WALK_SPLIT: the launch holds two kinds of workgroups and this walk covers one kind's tiles).
// An included text and not a function: hipcc's code for the body inlined from a function differs from its code for the same body in
// the kernel itself (register allocation and schedule), and the kernels of the 160^2 / 80^2 levels are to stay what they were.
// MT_ = 4: every tile is 16 rows high (16 | H).  MT_ = 2: the layers with H % 16 == 8 - the launch holds both walks, and a workgroup is
// of one kind for its whole life: groups of 8 workgroups (one per XCD, so every XCD gets the same mix) [0, wg8_full) walk the
// full-height tiles, the others the bottom tile row on 8-row tiles.  The branch is wave-uniform and sits in front of everything: no
// accumulator is live across it.  (the "; conv_xk walk" lines tell tools/check_xp_isa.py where a walk begins)
template <int NT_, int MT_, bool NORM, bool RES>
__global__ __launch_bounds__(XW_THREADS, 1) void conv_xk_kernel(const char* __restrict__ g_wpack, const ConvFFArgs k) {
  if constexpr (MT_ == 4) {
#define XK_WALK_MT 4
#define XK_WALK_SPLIT false
#include "conv_xk_walk.inc"
  } else if ((int)(blockIdx.x >> 3) < k.wg8_full) {
    asm volatile("; conv_xk walk MT = 4");
#define XK_WALK_MT 4
#define XK_WALK_SPLIT true
#include "conv_xk_walk.inc"
  } else {
    asm volatile("; conv_xk walk MT = 2");
#define XK_WALK_MT 2
#define XK_WALK_SPLIT true
#include "conv_xk_walk.inc"
  }
}

// What a bottom-row work item costs on an 8-row tile, as a fraction of a full-height item (the MFMA floor is 0.5; the conversion has 10 of
// 18 patch rows but two of three slots, the weight requests, the epilogue's rounds and the tile switch do not shrink).  Measured at 40^2,
// B = 64, from the per-tile cycle stamps of the tuning build (tools/xk_timing.py; "Half-height tiles" in profiles/NOTEBOOK.md): 0.686
// on a 192 -> 192 + residual layer (46.9 k of 68.3 k cycles), 0.639 on a 384 -> 192 layer (76.3 k of 119.3 k).  The split below is a
// matter of whole groups of 8 workgroups: at B = 64 any value in [0.64, 0.69] gives the same one.
static constexpr double XK_HALF_COST = 0.67;

// rounds of a walk: `items` spread over the 8 XCDs, each XCD's share over its wg8 workgroups
static int xk_rounds(int items, int wg8) { return wg8 > 0 ? ((items + 7) / 8 + wg8 - 1) / wg8 : 0; }

template <int NT, bool NORM, bool RES>
static int launch_xk(const ConvFFArgs& k0, hipStream_t s) {
  ConvFFArgs k = k0;
  const int n_cu = device_cu_count8();               // persistent: one workgroup per CU, a multiple of the 8 XCDs
  int grid = k.nblocks < n_cu ? (k.nblocks + 7) / 8 * 8 : n_cu;
  k.tpi_full = k.tpi; k.nblocks_full = k.nblocks; k.wg8_full = grid / 8;
  bool half = NT == 3 && k.H % FF_TILE == 8 && !CSD_TUNE_ENV("CSD_XK_NO_HALF");
  if (half) {
    // the bottom tile row on half-height tiles: split the workgroups between the two walks so that the longer one is as short as it
    // can be - full_items : XK_HALF_COST * half_items, in whole groups of 8.  Where every item has a workgroup of its own there is
    // nothing to balance.
    k.tpi_full = k.tpi - k.tiles_x;
    k.nblocks_full = k.B * k.tpi_full * k.n_groups;
    const int n_half = k.nblocks - k.nblocks_full;
    const int g8f = (k.nblocks_full + 7) / 8, g8h = (n_half + 7) / 8;
    if (8 * (g8f + g8h) <= n_cu) {
      k.wg8_full = g8f;
      grid = 8 * (g8f + g8h);
    } else {
      double best = 0.0;
      for (int h8 = 1; h8 < grid / 8; ++h8) {
        const double tf = xk_rounds(k.nblocks_full, grid / 8 - h8), th = XK_HALF_COST * xk_rounds(n_half, h8);
        const double t = tf > th ? tf : th;
        if (h8 == 1 || t < best) { best = t; k.wg8_full = grid / 8 - h8; }
      }
    }
  }
  if (half) {
    if constexpr (NT == 3) {
      auto kern = conv_xk_kernel<NT, 2, NORM, RES>;
      CSD_SET_MAX_LDS_ONCE(kern);
      hipLaunchKernelGGL(kern, dim3(grid), dim3(XW_THREADS), XKCfg<NT>::LDS, s, reinterpret_cast<const char*>(k.a.wpack), k);
    }
  } else {
    auto kern = conv_xk_kernel<NT, 4, NORM, RES>;
    CSD_SET_MAX_LDS_ONCE(kern);
    hipLaunchKernelGGL(kern, dim3(grid), dim3(XW_THREADS), XKCfg<NT>::LDS, s, reinterpret_cast<const char*>(k.a.wpack), k);
  }
  CSD_LAUNCH_CHECK();
  return CSD_OK;
}

// 96-cout groups and the 64-cout groups of the nf = 128 nets; at least three 16-channel stages; the packed weights are the Winograd
// layout of conv_ff.hip's convxw_pack_kernel
bool convxk_supported(const ConvFFArgs& k, int nt) { return (nt == 3 || nt == 2) && k.nstage >= 3; }

int convxk_launch(const ConvFFArgs& k, int nt, hipStream_t s) {
  const bool norm = k.a.nscale != nullptr, res = k.a.res != nullptr;
  if (nt == 2) {
    if (norm) return res ? launch_xk<2, true, true>(k, s) : launch_xk<2, true, false>(k, s);
    return res ? launch_xk<2, false, true>(k, s) : launch_xk<2, false, false>(k, s);
  }
  if (norm) return res ? launch_xk<3, true, true>(k, s) : launch_xk<3, true, false>(k, s);
  return res ? launch_xk<3, false, true>(k, s) : launch_xk<3, false, false>(k, s);
}

}  // namespace csd
