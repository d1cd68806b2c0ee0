// plan_common.h -- what every unit that reads a plan shares: the tuning constants, the tile descriptor, the device-side view
// of a plan and the device helpers of the kernels that walk one (LDS-DMA ring, unit tickets).  No kernels: those are in
// kernels_plan.h (construction, the DM steps), kernels_linear.h, kernels_cnn.h, kernels_evalplan.h, ...
#pragma once
#include "sorted_common.h"

#ifndef PLN_THREADS
#define PLN_THREADS 1024
#endif
#define PLN_WAVES (PLN_THREADS / 64)
#ifndef PLN_UNITS
#define PLN_UNITS 32                          // units per tile: two per wave, drawn dynamically, dearest first
#endif
#define PLN_NI (PLN_UNITS * 64)               // product-path items per tile (at most)
#ifndef PLN_NI_CUT
#define PLN_NI_CUT PLN_NI                      // ... that the greedy cut gives a tile
#endif
#ifndef PLN_RMAX
#define PLN_RMAX 1664                         // contexts per tile (at most; LDS)
#endif
#ifndef PLN_HCAP
#define PLN_HCAP 128                          // large-count items / contexts evaluated inside a tile (rest: global lists)
#endif
// Row totals n in (SRT_CL, PLN_NBIG] are ALSO counted in a histogram of the plan (bear_plan::hist + 2 SRT_NKEY, [n]): where every
// context shares its concentration total A (softmax rows: A = u + 5 eps; mode R always) the context term -D(A, n) is a function of n
// alone, and sum over rows = sum_n count[n] D(A, n) -- a few thousand Stirling evaluations per LAUNCH instead of one per row
// (5 % of the rows of the k = 13 table: a 64-lane unit of ~400 dependent instructions per tile, and 3.5e5 evaluations in the mode-R
// step of configs[1]).  The lists keep every such row (kernels with a concentration total per row read them as before); kernels
// that take the histogram skip the listed rows with n <= PLN_NBIG (round 6).
#define PLN_NBIG 4096
#define PLN_BLOCKS_PER_CU (1024 / PLN_THREADS)   // resident blocks of the planned step kernels per CU (LDS: 160 KB / that many)
#define PLN_QUAD 4                            // tiles start on multiples of 4 contexts (16-byte aligned rows)
#define PLN_LIVE_STRIDE (PLN_RMAX + 8)        // uint16 per tile of the live-context lists (a multiple of 8: 16-byte rows)
#define PLN_SENTINEL (PLN_RMAX * 5)           // flat offset of the neutral cell (prior = 1 / ref row = 0)
#ifndef PLN_NBUF
#define PLN_NBUF 2                            // LDS ring depth: tiles in flight = PLN_NBUF - 1
#endif
// bytes of one tile's plan block: E | nrow | items | heavy column items (off, c) | heavy contexts (row, n)
#define PLN_BLOCK_MAX (64 + PLN_RMAX + PLN_NI * 2 + PLN_HCAP * (2 + 4 + 2 + 8))

struct pln_tile {
  uint64_t row0;
  uint32_t rows_items;  // rows << 16 | n_light
  uint32_t off16;       // start of the tile's block in the plan stream, 16-byte units
  uint32_t hc_hr;       // in-tile large-count column items << 16 | in-tile large-total contexts
  uint32_t blk16;       // size of the block in 16-byte units
  uint64_t pad;
};
static_assert(sizeof(pln_tile) == 32, "tile descriptors are fetched with one s_load_dwordx8");
#ifndef PLN_CHUNK
#define PLN_CHUNK 128                       // contexts per wave pass of the row-sum check (two per lane)
#endif
#ifndef PLN_DMA_WAVES
#define PLN_DMA_WAVES 2                     // waves of each block that only stream tiles into LDS (see dm_prior_plan_kernel)
#endif
#ifndef PLN_PREFETCH_KIB
#define PLN_PREFETCH_KIB 24                 // L2 prefetch of the tile after next by the DMA waves of the light mode-N forms (0: off)
#endif
// General mode-N form (rows not asserted normalised) of dm_prior_plan_kernel, switches for A/B builds:
#ifndef PLN_GEN_PREFETCH
#define PLN_GEN_PREFETCH 1                  // 1: the L2 prefetch of the tile after next there too
#endif
#ifndef PLN_GEN_NT
#define PLN_GEN_NT 0                        // 1: the ring's LDS-DMA loads (prior rows, plan blocks) with the non-temporal policy
#endif
#ifndef PLN_GEN_NROW_ON_DEMAND
#define PLN_GEN_NROW_ON_DEMAND 1            // 1: a tile's nrow bytes are staged only behind a tile with a failing row sum
#endif
#define PLN_DESC_CHUNK 32                   // descriptors per 1 KiB LDS-DMA piece
#define PLN_DESC_PAD (2 * PLN_DESC_CHUNK)   // zeroed descriptors behind the last tile (plan allocation)

struct pln_layout {  // byte offsets inside a tile's block (all multiples of 16)
  uint32_t nrow, items, hoff, hcnt, hrow, hn, end;
};
__host__ __device__ inline pln_layout pln_block_layout(uint32_t rows, uint32_t n_light, uint32_t hc, uint32_t hr) {
  pln_layout L;
  L.nrow = 64u;
  L.items = L.nrow + ((rows + 15u) & ~15u);
  L.hoff = L.items + (((n_light + 63u) & ~63u) * 2u);
  L.hcnt = L.hoff + (((hc + 7u) & ~7u) * 2u);
  L.hrow = L.hcnt + (((hc + 3u) & ~3u) * 4u);
  L.hn = L.hrow + (((hr + 7u) & ~7u) * 2u);
  L.end = L.hn + (((hr + 1u) & ~1u) * 8u);
  return L;
}

struct pln_heavy_col {
  uint64_t off;  // flat offset row*5+b into the [N,5] arrays
  uint64_t c;
};

struct pln_heavy_row {
  uint64_t row;
  double n;  // exact row total (may exceed 2^32)
};

struct pln_view {  // device-side view of a plan
  const pln_tile *tiles;
  const unsigned char *stream;
  const pln_heavy_col *heavy_col;
  const pln_heavy_row *heavy_row;
  const uint64_t *heavy_stop;
  const unsigned long long *hist;  // [0..31] contexts with total n = j+1, [32..63] with stop count j+1 (<= SRT_CL)
  const unsigned long long *hist_big;   // [n], SRT_CL < n <= PLN_NBIG: contexts with that total (also in the lists); NULL: this launch does not add them
  int big_in_hist;                 // the listed rows with a total <= PLN_NBIG are accounted for by the histogram (this launch's, or -- a
                                   // step of two launches over subsets of the tiles -- its sibling's): kernels that take it skip them
  uint64_t n_tiles, n_heavy_col, n_heavy_row, n_heavy_stop;
  const uint16_t *live;            // [n_tiles][PLN_LIVE_STRIDE] (five-column plans): [0] = contexts with counts, then their rows, ascending
  const uint16_t *live2;           // [n_tiles][LIN_LIVE2_STRIDE] or NULL: the paired form of `live` for one set of k-mers (kernels_linear.h)
  int subset;                      // `tiles` is a subset of the plan's tiles: a descriptor's spare word holds (tile number << 32 | list length)
};

// Context terms of the rows with a total in (SRT_CL, PLN_NBIG] from the plan's histogram, for kernels whose contexts share the
// concentration total A: acc_D -= m D(A, n), acc_P += scale m P(A, n), the bins dealt over the launch's threads.
__device__ __forceinline__ void pln_big_totals(const pln_view &pv, double A, double scale, uint64_t gtid, uint64_t gsz, const double2 *logtab,
                                               double &acc_D, double &acc_P) {
  if (!pv.hist_big) return;
  for (uint64_t n = SRT_CL + 1 + gtid; n <= PLN_NBIG; n += gsz) {
    const unsigned long long m = pv.hist_big[n];
    if (m) {
      const bear_dp o = srt_general_fast(A, (double)n, logtab);
      acc_D -= (double)m * o.D;
      acc_P = __builtin_fma(scale * (double)m, o.P, acc_P);
    }
  }
}
// ... and whether a listed row is one of them (then the histogram has it)
__device__ __forceinline__ bool pln_in_big_hist(const pln_view &pv, double n) { return pv.big_in_hist && n <= (double)PLN_NBIG; }

// DMA of `bytes` (multiple of 16) to LDS: 1 KiB pieces round-robin over the waves starting at wave
// `first` (so successive slabs spread over different waves), the last piece with surplus lanes masked.
// Returns the number of DMA instructions this wave issued.  Inline asm on purpose: see kernels_sorted.h.
__device__ __forceinline__ uint32_t pln_dma(void *lds, const void *src, uint32_t bytes, uint32_t wave, uint32_t lane,
                                            uint32_t first) {
  const uint32_t d = (uint32_t)(uintptr_t)lds;
  const unsigned char *s = static_cast<const unsigned char *>(src) + lane * 16u;
  const uint32_t pieces = (bytes + 1023u) >> 10;
  uint32_t issued = 0;
  for (uint32_t piece = (wave + PLN_WAVES - (first % PLN_WAVES)) % PLN_WAVES; piece < pieces; piece += PLN_WAVES) {
    const unsigned char *g = s + (piece << 10);
    const uint32_t m = srt_uniform(d + (piece << 10));
    if ((piece << 10) + lane * 16u < bytes)
      {
      // M0 is compiler-reserved: saved and restored inside the statement that uses it (no "m0" clobber: that is undefined behaviour)
      uint32_t keep_m0;
      asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                   : "=&s"(keep_m0)
                   : "v"(g), "s"(m)
                   : "memory");
    }
    ++issued;
  }
  return issued;
}

// One 1 KiB piece (`piece` = KiB index inside a slab of `bytes` bytes, multiple of 16) as a single DMA instruction.
// NT: the non-temporal policy (bytes read once per launch, far more of them than the caches hold).
template <bool NT = false>
__device__ __forceinline__ void pln_dma_piece(void *lds, const void *src, uint32_t bytes, uint32_t piece, uint32_t lane) {
  const uint32_t m = srt_uniform((uint32_t)(uintptr_t)lds + (piece << 10));
  const unsigned char *g = static_cast<const unsigned char *>(src) + (piece << 10) + lane * 16u;
  if ((piece << 10) + lane * 16u < bytes)
    {
      // M0 is compiler-reserved: saved and restored inside the statement that uses it (no "m0" clobber: that is undefined behaviour)
      uint32_t keep_m0;
      if (NT)
        asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off nt\n\ts_mov_b32 m0, %0"
                     : "=&s"(keep_m0)
                     : "v"(g), "s"(m)
                     : "memory");
      else
        asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                     : "=&s"(keep_m0)
                     : "v"(g), "s"(m)
                     : "memory");
    }
}

// Waits until at most `younger` of this wave's vector-memory operations are outstanding (vmcnt is an
// immediate, hence the ladder; a wave issues at most 3 DMA pieces per tile).
__device__ __forceinline__ void pln_wait_all_but(uint32_t younger) {
  switch (younger) {
    case 0: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
    case 1: asm volatile("s_waitcnt vmcnt(1)" ::: "memory"); break;
    case 2: asm volatile("s_waitcnt vmcnt(2)" ::: "memory"); break;
    case 3: asm volatile("s_waitcnt vmcnt(3)" ::: "memory"); break;
    case 4: asm volatile("s_waitcnt vmcnt(4)" ::: "memory"); break;
    case 5: asm volatile("s_waitcnt vmcnt(5)" ::: "memory"); break;
    case 6: asm volatile("s_waitcnt vmcnt(6)" ::: "memory"); break;
    case 7: asm volatile("s_waitcnt vmcnt(7)" ::: "memory"); break;
    case 8: asm volatile("s_waitcnt vmcnt(8)" ::: "memory"); break;
    default: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
  }
}

// Scalar (s_load) fetch of a tile descriptor: a vector-memory load here would make the compiler
// wait for vmcnt(0) at its first use -- and vmcnt is in order, so that wait would drain the DMA ring.
__device__ __forceinline__ pln_tile pln_load_tile(const pln_view &pv, uint64_t t) {
  pln_tile ti;
  ti.row0 = 0;
  ti.rows_items = 0;
  ti.off16 = 0;
  ti.hc_hr = 0;
  ti.blk16 = 0;
  ti.pad = 0;
  if (t < pv.n_tiles) {
    const __attribute__((address_space(4))) pln_tile *tc = (const __attribute__((address_space(4))) pln_tile *)(uintptr_t)pv.tiles;
    ti.row0 = tc[t].row0;
    ti.rows_items = tc[t].rows_items;
    ti.off16 = tc[t].off16;
    ti.hc_hr = tc[t].hc_hr;
    ti.blk16 = tc[t].blk16;
    ti.pad = tc[t].pad;       // (subset launches of the linear step, kernels_linear.h; zero in the plan's own array)
  }
  return ti;
}

// Dynamic work distribution inside a tile: every wave draws tickets from an LDS counter.
// Lane 0's `ds_add_rtn_u32` is spelled out: of an atomicAdd under `if (lane == 0)` the compiler makes its wave-aggregated form
// (count the active lanes with v_mbcnt x 2 + s_bcnt1, elect one, add the count, hand every lane its own offset: nine vector
// instructions and the LDS one), which a draw by one known lane does not need.  All 64 lanes are active at every call.
__device__ __forceinline__ uint32_t pln_ticket(uint32_t *counter, uint32_t lane) {
  uint32_t t = 0;
  if (lane == 0)
    asm volatile("ds_add_rtn_u32 %0, %1, %2\n\ts_waitcnt lgkmcnt(0)" : "=&v"(t) : "v"((uint32_t)(uintptr_t)counter), "v"(1u) : "memory");
  return srt_uniform(t);
}

// Work units of a tile are DRAWN: whichever wave is free takes the next one, so which thread accumulates which items changes from
// run to run and the fp64 sums of a launch are reproducible to rounding only (their order across blocks is fixed).  The
// deterministic build (-DBEAR_DET_BUILD: libbear_hip_det.so, loaded when BEAR_AMD_DETERMINISTIC is set at import) deals them
// out instead: drawing wave `first` of `stride` takes units first, first + stride, ... -- every sum is then bit-identical from
// run to run, at the price of the dynamic balance.
#ifdef BEAR_DET_BUILD
#define PLN_FOR_UNITS(w, counter, n, first, stride) for (uint32_t w = (first); w < (n); w += (stride))
#else
#define PLN_FOR_UNITS(w, counter, n, first, stride) for (uint32_t w = pln_ticket(counter, lane); w < (n); w = pln_ticket(counter, lane))
#endif
// The same with a wave's FIRST unit dealt (drawing wave `first` of `stride` starts with unit `first`, the counter starts at `stride`:
// PLN_TICKET_START): one LDS atomic round trip less per wave and tile.
#if defined(BEAR_DET_BUILD) || defined(PLN_NO_FIRST_UNIT_DEALT)
#define PLN_FOR_UNITS_F(w, counter, n, first, stride) PLN_FOR_UNITS(w, counter, n, first, stride)
#define PLN_TICKET_START(stride) 0u
#else
#define PLN_FOR_UNITS_F(w, counter, n, first, stride) for (uint32_t w = (first); w < (n); w = pln_ticket(counter, lane))
#define PLN_TICKET_START(stride) ((uint32_t)(stride))
#endif

// (Round 6, measured and not kept: the NEXT ticket drawn in front of the current unit -- the draw's LDS round trip, ~1000 clocks on a
// CU whose LDS queue the units keep busy, then hides behind the unit -- made the linear step 4.7 % SLOWER, 0.902 against 0.861 ms:
// a wave holds the phase's last units while others idle at the barrier.  The evaluation kernel had found the same in round 4.)
// The same draw without waiting for its answer: lane 0's return value, to be made uniform (srt_uniform) when it is looked at.
__device__ __forceinline__ uint32_t pln_ticket_issue(uint32_t *counter, uint32_t lane) {
  uint32_t t = 0;
  if (lane == 0) t = atomicAdd(counter, 1u);
  return t;
}

// Counts of the 64 items of unit `un` from the tile's thresholds: an item's count is the number of
// thresholds E[c] that do not exceed its index.  Returns the lane's count (0 beyond n_light) and the
// wave-uniform range of the unit.
__device__ __forceinline__ uint32_t pln_unit_counts(const uint16_t *E, uint32_t n_light, uint32_t un, uint32_t lane,
                                                    uint32_t *cmin, uint32_t *cmax) {
  const uint32_t base = un * 64u, idx = base + lane;
  const uint32_t last = (base + 64u <= n_light ? base + 64u : n_light) - 1u;  // last occupied index (unit not empty)
  const uint32_t e = lane < 30u ? (uint32_t)E[lane] : 0xffffffffu;  // E[30], E[31]: heavy list lengths
  // (s_bcnt1 by name: the 32-bit results of __builtin_popcountll stay 64-bit values to the compiler, and with no scalar 64-bit
  // "less than" the loop test below became a v_cmp_ge_u64 behind two moves)
  uint32_t lo, hi;
  asm("s_bcnt1_i32_b64 %0, %1" : "=s"(lo) : "s"(__builtin_amdgcn_ballot_w64(e <= base)) : "scc");
  asm("s_bcnt1_i32_b64 %0, %1" : "=s"(hi) : "s"(__builtin_amdgcn_ballot_w64(e <= last)) : "scc");
  uint32_t c = lo;
  for (uint32_t k = lo; k < hi; ++k) c += idx >= (uint32_t)__builtin_amdgcn_readlane((int)e, (int)k) ? 1u : 0u;
  *cmin = base + 64u <= n_light ? lo : 0u;  // un-predicated factors only in full units
  *cmax = hi;
  return idx < n_light ? c : 0u;
}

// ---- mode N ---------------------------------------------------------------------------------
struct pln_buf_n {
  double pri[PLN_RMAX * 5 + 2];                      // [PLN_SENTINEL] = 1.0
  __attribute__((aligned(16))) unsigned char blk[PLN_BLOCK_MAX];  // E[32] u16 | nrow u8[rows~16] | items u16[n_light~64]
};
struct pln_lds_n {
  pln_buf_n buf[PLN_NBUF];
  double2 logtab[BEAR_LOGTAB_N];
  double tabD[SRT_NKEY];  // D(u + 5 eps, j + 1)
  double tabP[SRT_NKEY];
  uint32_t ticket[PLN_NBUF];  // per ring slot; zeroed one tile ahead
  uint32_t sum_fail[PLN_NBUF];   // general form: the tile in the slot holds a row whose sum fails the test (set by compute waves)
  uint32_t nrow_in[PLN_NBUF];    // general form: the tile in the slot was staged with its nrow range (set by the DMA waves)
  __attribute__((aligned(16))) pln_tile desc[2][PLN_DESC_CHUNK];  // descriptors of this block's tile range, 2 x 32
  __attribute__((aligned(16))) uint32_t pf_scratch[64];           // where the L2 prefetch's dwords land (never read)
};
static_assert(sizeof(pln_lds_n) <= 160 * 1024, "one block per CU: the planned mode-N kernels' LDS");

// Tile descriptor j of the block's range from the LDS ring (wave-uniform: every lane reads the same address).
__device__ __forceinline__ pln_tile pln_desc(const pln_tile (*ring)[PLN_DESC_CHUNK], uint64_t j, uint64_t count) {
  pln_tile ti;
  ti.row0 = 0;
  ti.rows_items = 0;
  ti.off16 = 0;
  ti.hc_hr = 0;
  ti.blk16 = 0;
  ti.pad = 0;
  if (j < count) {
    const uint32_t *d = reinterpret_cast<const uint32_t *>(&ring[(j >> 5) & 1u][j & 31u]);
    const uint32_t lo = srt_uniform(d[0]), hi = srt_uniform(d[1]);
    ti.row0 = ((uint64_t)hi << 32) | lo;
    ti.rows_items = srt_uniform(d[2]);
    ti.off16 = srt_uniform(d[3]);
    ti.hc_hr = srt_uniform(d[4]);
    ti.blk16 = srt_uniform(d[5]);
  }
  return ti;
}

// a wave-uniform look at an LDS word that other waves of the block advance (ring hand-over counters)
__device__ __forceinline__ uint32_t pln_peek(const uint32_t *p) {
  return srt_uniform(__hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP));
}
