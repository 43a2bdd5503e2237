// clrrt_occ.hpp -- the static occupancy grid of CLRRT_COLLISION_OCC: the bake kernels (cell bytes -> bit-packed
// occupancy map + conservative reach map) and the per-step test of the rollout kernels.
//
// The decision (include/clrrt.h, clrrt_set_occupancy): with vp the vehicle box centre, (cs, sn) the heading's cosine
// and sine, c the centre of an occupied cell, d = c - vp, u = d.x cs + d.y sn, v = d.y cs - d.x sn, the grid hits when
// some occupied cell has |u| <= 2.424 + inflate and |v| <= 1 + inflate, all in double.  A non-finite vp or heading does
// not hit.
//
// A stack of layers (clrrt_set_occupancy_layers) is `layers` such grids of one geometry, one per time slice: the bake
// kernels take the layer from blockIdx.y, and a step tests the maps of the layer occ_layer gives for its time.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "clrrt_internal.hpp"

namespace clrrt {

#define OCC_VEH_A 2.424 /* vehicle box half length (old_collisioncheck.cpp:34-36) */
#define OCC_VEH_B 1.0   /* half width */

// ------------------------------------------------------------------------------------------------ bake
// Bytes -> bits: one lane per cell of a row padded to 64 cells (ws is even), so a wave's ballot is two whole words of
// one row, stored by its first lane; the padding bits are 0.  The occupied cells of layer blockIdx.y are counted into
// count[blockIdx.y]; ostride: words per layer of occ.
__global__ void __launch_bounds__(256) k_occ_pack(const uint8_t* __restrict__ cells, int w, int h, int ws, int ostride,
                                                  uint32_t* __restrict__ occ, unsigned int* __restrict__ count) {
  cells += (int64_t)blockIdx.y * w * h;
  occ += (int64_t)blockIdx.y * ostride;
  count += blockIdx.y;
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int rowbits = ws * 32;
  const int64_t j = idx / rowbits;
  const int i = (int)(idx % rowbits);
  const bool on = j < h && i < w && cells[j * w + i] != 0;
  const unsigned long long m = __ballot(on);
  if ((threadIdx.x & 63) == 0 && j < h) {
    uint32_t* o = occ + j * ws + (i >> 5);
    o[0] = (uint32_t)m;
    o[1] = (uint32_t)(m >> 32);
    if (m) atomicAdd(count, (unsigned int)__popcll(m));
  }
}

// The reach map.  Reach cell (ri, rj) is the square of rk x rk occupancy cells whose corner is cell
// ((ri - rm) rk, (rj - rm) rk); in units of one occupancy cell from the grid's corner (x0, y0) it is
// [ax, ax + rk] x [ay, ay + rk] with integers ax, ay, and the centre of cell (i, j) is (i + 0.5, j + 0.5).  Its bit is
// set when some occupied centre lies within Rc (cells) of the square.
//
// Why the clear bits are safe (a superset of the states that can hit): a hit needs an occupied centre c with
// |u| <= A + inflate and |v| <= B + inflate, so |c - vp| <= |(A, B) + inflate (1, 1)| <= sqrt(A^2 + B^2) + inflate
// sqrt 2 = R.  A vp inside the square is then within R of c, so the square is within R of c.  Rc = (R + slack) / res
// with slack = res / 64 + 1e-9 (|x0| + |y0| + the map's extent), far above what rounding can move: the step's lookup
// floor((vp - rx0) / rres) and the cell centres x0 + (i + 0.5) res are each off by a few ulps of the coordinates
// (clrrt_set_occupancy refuses a grid whose res is below 2^-30 of them).  The scan below visits a superset of the
// centres within Rc of the square: every row whose centre line is within Rc of [ay, ay + rk] (one row of slack either
// side), and on a row at distance dy the columns within sqrt(Rc^2 - dy^2) of [ax, ax + rk] (one column of slack).
// A vp outside the map is more than rm rk >= Rc + rk cells from every centre: free.
// Layer blockIdx.y: ostride / rstride words per layer of occ / reach.
__global__ void __launch_bounds__(256) k_occ_reach(const uint32_t* __restrict__ occ, int w, int h, int ws, int rk, int rm,
                                                   double Rc, int rw, int rh, int rws, int ostride, int rstride,
                                                   uint32_t* __restrict__ reach) {
  occ += (int64_t)blockIdx.y * ostride;
  reach += (int64_t)blockIdx.y * rstride;
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int rowbits = rws * 32;
  const int64_t rj = idx / rowbits;
  const int ri = (int)(idx % rowbits);
  bool on = false;
  if (rj < rh && ri < rw) {
    const double ax = (double)(ri - rm) * rk, ay = (double)(rj - rm) * rk;
    const double jlo = floor(ay - Rc - 0.5) - 1.0, jhi = ceil(ay + rk + Rc - 0.5) + 1.0;
    const int j0 = (int)fmax(jlo, 0.0), j1 = (int)fmin(jhi, (double)(h - 1));
    for (int j = j0; j <= j1 && !on; j++) {
      const double y = j + 0.5;
      const double dy = fmax(fmax(ay - y, y - (ay + rk)), 0.0);
      const double s2 = Rc * Rc - dy * dy;
      const double span = s2 > 0.0 ? sqrt(s2) : 0.0;  // (a slack row: its nearest columns only)
      const double ilo = floor(ax - span - 0.5) - 1.0, ihi = ceil(ax + rk + span - 0.5) + 1.0;
      if (ihi < 0.0 || ilo > (double)(w - 1)) continue;
      const int i0 = (int)fmax(ilo, 0.0), i1 = (int)fmin(ihi, (double)(w - 1));
      const uint32_t* row = occ + (int64_t)j * ws;
      for (int q = i0 >> 5; q <= (i1 >> 5); q++) {
        uint32_t m = row[q];
        if (q == (i0 >> 5)) m &= ~0u << (i0 & 31);
        if (q == (i1 >> 5)) m &= ~0u >> (31 - (i1 & 31));
        if (m) { on = true; break; }
      }
    }
  }
  const unsigned long long m = __ballot(on);
  if ((threadIdx.x & 63) == 0 && rj < rh) {
    uint32_t* o = reach + rj * rws + (ri >> 5);
    o[0] = (uint32_t)m;
    o[1] = (uint32_t)(m >> 32);
  }
}

// The union reach map of a stack: word q of uni is the bitwise OR of word q of every layer's reach map (n words per
// layer, rstride apart).
//
// Why its clear bits are safe for every layer (a superset of a superset): layer k's reach map has a set bit wherever a
// state can hit layer k (k_occ_reach's argument), so a bit that is clear in the OR is clear in every layer's map and
// no state in that reach cell hits any layer -- whichever layer the step's time selects.  The step may therefore take
// a clear union bit as free without knowing its layer; a set bit decides nothing and the layer's own maps follow.
__global__ void __launch_bounds__(256) k_occ_reach_union(const uint32_t* __restrict__ reach, int n, int rstride,
                                                         int layers, uint32_t* __restrict__ uni) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= n) return;
  uint32_t m = 0u;
  for (int k = 0; k < layers; k++) m |= reach[(int64_t)k * rstride + q];
  uni[q] = m;
}

// ------------------------------------------------------------------------------------------------ distance field
// The squared Euclidean distance field of clrrt_set_occupancy_clearance: field[j w + i] = min over occupied cells
// (i', j') of (i - i')^2 + (j - j')^2, exact in uint32 (at most 2 * 2047^2), OCC_FIELD_NONE without an occupied cell.
// Separable: the row pass writes each cell's distance to the nearest occupied cell of its own row, the column pass
// takes min over rows j' of (j - j')^2 + rowd[j'][i]^2.
#define OCC_FIELD_NONE 0xFFFFFFFFu
#define OCC_ROWD_NONE 0xFFFFu

// Row pass, one lane per cell of a row padded to 64 cells as in k_occ_pack.  A row has at most 64 words, so lane q of
// every wave holds word q of the wave's row and the ballot of the non-zero ones; a cell's nearest occupied cell on
// either side is in its own word (clz / ctz of the masked word) or in the nearest non-zero word on that side (clz /
// ctz of the ballot, the word fetched by a shuffle).  The padding bits are 0.  Rows with an occupied cell are marked
// in rowmask (bit j & 31 of word j >> 5).  Layer blockIdx.y: ostride words of occ, w h entries of rowd and 64 words
// of rowmask per layer.
__global__ void __launch_bounds__(256) k_occ_field_rows(const uint32_t* __restrict__ occ, int w, int h, int ws, int ostride,
                                                        uint16_t* __restrict__ rowd, uint32_t* __restrict__ rowmask) {
  occ += (int64_t)blockIdx.y * ostride;
  rowd += (int64_t)blockIdx.y * w * h;
  rowmask += blockIdx.y * 64;
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int rowbits = ws * 32;
  const int64_t j = idx / rowbits;
  const int i = (int)(idx % rowbits);
  if (j >= h) return;  // (wave-uniform: a wave lies in one row)
  const int lane = threadIdx.x & 63;
  const uint32_t word = lane < ws ? occ[j * ws + lane] : 0u;
  const unsigned long long nz = __ballot(word != 0u);
  if (i == 0 && nz) atomicOr(&rowmask[j >> 5], 1u << (j & 31));
  const int qi = i >> 5, b = i & 31;
  const uint32_t own = (uint32_t)__shfl((int)word, qi, 64);
  const uint32_t ml = own & (~0u >> (31 - b));  // occupied cells of the own word at or left of i
  const uint32_t mr = own & (~0u << b);         // at or right of i
  const unsigned long long nzl = nz & ((1ull << qi) - 1ull);
  const unsigned long long nzr = qi >= 63 ? 0ull : nz & (~0ull << (qi + 1));
  const int ql = nzl ? 63 - __clzll((long long)nzl) : 0;
  const int qr = nzr ? __ffsll((long long)nzr) - 1 : 0;
  const uint32_t wl = (uint32_t)__shfl((int)word, ql, 64);
  const uint32_t wr = (uint32_t)__shfl((int)word, qr, 64);
  int dl = (int)OCC_ROWD_NONE, dr = (int)OCC_ROWD_NONE;
  if (ml) dl = b - (31 - __clz((int)ml));
  else if (nzl) dl = i - (ql * 32 + 31 - __clz((int)wl));
  if (mr) dr = (__ffs((int)mr) - 1) - b;
  else if (nzr) dr = qr * 32 + (__ffs((int)wr) - 1) - i;
  if (i < w) rowd[j * w + i] = (uint16_t)min(dl, dr);
}

// The nearest non-empty row at or below / at or above j (-1: none); nw = words of the mask.
__device__ __forceinline__ int occ_row_prev(const uint32_t* __restrict__ m, int j) {
  int q = j >> 5;
  uint32_t x = m[q] & (~0u >> (31 - (j & 31)));
  while (!x) {
    if (--q < 0) return -1;
    x = m[q];
  }
  return q * 32 + 31 - __clz((int)x);
}
__device__ __forceinline__ int occ_row_next(const uint32_t* __restrict__ m, int j, int nw) {
  int q = j >> 5;
  uint32_t x = m[q] & (~0u << (j & 31));
  while (!x) {
    if (++q >= nw) return -1;
    x = m[q];
  }
  return q * 32 + __ffs((int)x) - 1;
}

// Column pass, one lane per cell, adjacent lanes on adjacent columns (the loads of a row coalesce): a windowed
// minimum over the non-empty rows, outward from the cell's own row in both directions, that stops where (j - j')^2
// alone reaches the best so far -- no row farther out can lower it.  The row skip makes a nearly empty map (the
// window's worst case) cost a few rows per cell.  Layer blockIdx.y: w h entries of rowd, 64 words of rowmask and
// fstride dwords of field per layer.
__global__ void __launch_bounds__(256) k_occ_field_cols(const uint16_t* __restrict__ rowd,
                                                        const uint32_t* __restrict__ rowmask, int w, int h, int fstride,
                                                        uint32_t* __restrict__ field) {
  rowd += (int64_t)blockIdx.y * w * h;
  rowmask += blockIdx.y * 64;
  field += (int64_t)blockIdx.y * fstride;
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (int64_t)w * h) return;
  const int j = (int)(idx / w), i = (int)(idx % w);
  const int nw = (h + 31) >> 5;
  uint32_t best = OCC_FIELD_NONE;
  const uint32_t g0 = rowd[idx];
  if (g0 != OCC_ROWD_NONE) best = g0 * g0;
  for (int jj = j - 1; jj >= 0; jj--) {
    jj = occ_row_prev(rowmask, jj);
    if (jj < 0) break;
    const uint32_t d = (uint32_t)(j - jj);
    if (d * d >= best) break;
    const uint32_t g = rowd[(int64_t)jj * w + i];  // (a marked row has a distance in every cell)
    best = min(best, d * d + g * g);
  }
  for (int jj = j + 1; jj < h; jj++) {
    jj = occ_row_next(rowmask, jj, nw);
    if (jj < 0) break;
    const uint32_t d = (uint32_t)(jj - j);
    if (d * d >= best) break;
    const uint32_t g = rowd[(int64_t)jj * w + i];
    best = min(best, d * d + g * g);
  }
  field[idx] = best;
}

// ------------------------------------------------------------------------------------------------ step test
// The maps a kernel reads: the grid record (a kernel argument: scalar loads) and the two bitmaps, in LDS
// (occ_stage) or global memory; scans counts the lane's steps that took the exact scan.  uni: the union reach map in
// LDS where the launch staged it alone (OCC_IN_LDS_UNION), else null.
struct OccView {
  const OccGrid* g;
  const uint32_t* occ;
  const uint32_t* reach;
  uint32_t scans;
  const uint32_t* uni;
};

// The layer of a step at time t (include/clrrt.h, clrrt_set_occupancy_layers): q = (t - t0) / dt in double (a
// division); layer 0 when !(q >= 0) (times before t0, NaN, -inf), the last layer when q >= layers - 1 (+inf too),
// (int)q between.  One layer: 0 by the same rule, without the arithmetic.
__device__ __forceinline__ int occ_layer(const OccGrid& g, double t) {
  if (g.layers <= 1) return 0;
  const double q = (t - g.t0) / g.dt;
  if (!(q >= 0.0)) return 0;
  if (q >= (double)(g.layers - 1)) return g.layers - 1;
  return (int)q;
}

// Copies the maps into the block's dynamic LDS at g.lds_off when the launch placed them there -- every layer's two
// bitmaps (OCC_IN_LDS), or the union reach map alone (OCC_IN_LDS_UNION) -- (every thread of the block calls it; the
// caller's next barrier, or this one, orders the copy before the first step).
// LAYERED: the instantiation serves a stack of more than one layer (the launch picks it by g.layers); without it the
// code is the single grid's -- no layer arithmetic, no strides, no union map.
template <bool LAYERED>
__device__ __forceinline__ OccView occ_stage(const OccGrid& g, void* lds_base) {
  OccView v{&g, g.occ, g.reach, 0u, nullptr};
  if (g.in_lds == OCC_IN_LDS) {
    uint32_t* o = (uint32_t*)((char*)lds_base + g.lds_off);
    const int no = LAYERED ? g.layers * g.occ_stride : g.h * g.ws, nr = LAYERED ? g.layers * g.reach_stride : g.rh * g.rws;
    for (int q = threadIdx.x; q < no; q += blockDim.x) o[q] = g.occ[q];
    for (int q = threadIdx.x; q < nr; q += blockDim.x) o[no + q] = g.reach[q];
    __syncthreads();
    v.occ = o;
    v.reach = o + no;
  } else if (LAYERED && g.in_lds == OCC_IN_LDS_UNION) {
    uint32_t* o = (uint32_t*)((char*)lds_base + g.lds_off);
    const int nr = g.reach_stride;
    for (int q = threadIdx.x; q < nr; q += blockDim.x) o[q] = g.reach_u[q];
    __syncthreads();
    v.uni = o;
  }
  return v;
}

// One step's grid decision against layer k for the vehicle box centre (vpx, vpy) and heading th with cosine cs and
// sine sn: the reach-map bit at vp (clear: free, the open-space path), else the occupied cells inside the axis-aligned
// bounds of the inflated box (one cell of slack: the exact test below decides), taken word by word and bit by bit.
// Where the launch staged the union reach map alone, its bit in LDS comes first (clear: free for every layer, no
// global memory touched), then the layer's reach bit and occupancy words in global memory.
template <bool LAYERED>
__device__ __forceinline__ bool occ_hit(OccView& ov, int k, double vpx, double vpy, double th, double cs, double sn) {
  const OccGrid& g = *ov.g;
  if (!(isfinite(vpx) && isfinite(vpy) && isfinite(th))) return false;
  const double fx = (vpx - g.rx0) / g.rres, fy = (vpy - g.ry0) / g.rres;
  if (!(fx >= 0.0 && fx < (double)g.rw && fy >= 0.0 && fy < (double)g.rh)) return false;
  const int ix = (int)fx, iy = (int)fy;
  const int rq = iy * g.rws + (ix >> 5);
  if constexpr (LAYERED)
    if (ov.uni && !((ov.uni[rq] >> (ix & 31)) & 1u)) return false;
  if (!((ov.reach[(LAYERED ? k * g.reach_stride : 0) + rq] >> (ix & 31)) & 1u)) return false;
  ov.scans++;
  const uint32_t* const occ = LAYERED ? ov.occ + k * g.occ_stride : ov.occ;
  const double A = OCC_VEH_A + g.inflate, B = OCC_VEH_B + g.inflate;
  const double ex = fabs(cs) * A + fabs(sn) * B, ey = fabs(sn) * A + fabs(cs) * B;
  // (vp lies inside the reach map, so these quotients are small numbers: the casts are in range)
  const double ilo = floor((vpx - ex - g.x0) / g.res - 0.5) - 1.0, ihi = ceil((vpx + ex - g.x0) / g.res - 0.5) + 1.0;
  const double jlo = floor((vpy - ey - g.y0) / g.res - 0.5) - 1.0, jhi = ceil((vpy + ey - g.y0) / g.res - 0.5) + 1.0;
  if (ihi < 0.0 || jhi < 0.0 || ilo > (double)(g.w - 1) || jlo > (double)(g.h - 1)) return false;
  const int i0 = (int)fmax(ilo, 0.0), i1 = (int)fmin(ihi, (double)(g.w - 1));
  const int j0 = (int)fmax(jlo, 0.0), j1 = (int)fmin(jhi, (double)(g.h - 1));
  for (int j = j0; j <= j1; j++) {
    const double dy = (g.y0 + (j + 0.5) * g.res) - vpy;
    const uint32_t* row = occ + j * g.ws;
    for (int q = i0 >> 5; q <= (i1 >> 5); q++) {
      uint32_t m = row[q];
      if (q == (i0 >> 5)) m &= ~0u << (i0 & 31);
      if (q == (i1 >> 5)) m &= ~0u >> (31 - (i1 & 31));
      while (m) {
        const int i = q * 32 + __builtin_ctz(m);
        m &= m - 1;
        const double dx = (g.x0 + (i + 0.5) * g.res) - vpx;
        const double u = dx * cs + dy * sn, v = dy * cs - dx * sn;
        if (fabs(u) <= A && fabs(v) <= B) return true;
      }
    }
  }
  return false;
}

// One step's clearance from layer k of the distance field g.field (non-null; include/clrrt.h, clrrt_set_occupancy_clearance):
// three circles of radius OCC_CLR_RC along the heading cover the vehicle box; each centre inside the grid reads its
// cell's squared distance (one dword from global memory), the smallest one gives the distance -- sqrt and the
// product with res are monotonic, so the minimum is taken over the integers -- and a centre outside the grid, a
// non-finite state or a map without an occupied cell leaves +inf, which the cap turns into clear_max.  All in double.
#define OCC_CLR_RC 1.2857 /* circle radius: half width 1 and a third of the half length, 0.808, under one hypotenuse */
#define OCC_CLR_S 1.616   /* spacing of the circle centres along the box axis */
template <bool LAYERED>
__device__ __forceinline__ double occ_clearance(const OccGrid& g, int layer, double vpx, double vpy, double th, double cs,
                                                double sn) {
  uint32_t m = OCC_FIELD_NONE;
  const uint32_t* const field = LAYERED ? g.field + (int64_t)layer * g.field_stride : g.field;
  if (isfinite(vpx) && isfinite(vpy) && isfinite(th)) {
#pragma unroll
    for (int k = -1; k <= 1; k++) {
      const double px = k ? vpx + (k * OCC_CLR_S) * cs : vpx, py = k ? vpy + (k * OCC_CLR_S) * sn : vpy;
      const double fx = (px - g.x0) / g.res, fy = (py - g.y0) / g.res;
      if (fx >= 0.0 && fx < (double)g.w && fy >= 0.0 && fy < (double)g.h) m = min(m, field[(int)fy * g.w + (int)fx]);
    }
  }
  const double d = m == OCC_FIELD_NONE ? (double)INFINITY : g.res * sqrt((double)m);
  double c = d - (OCC_CLR_RC + g.inflate);
  c = fmin(c, g.clear_max);
  return fmax(c, 0.0);
}

// The value the obstacle cost term takes for a step that does not collide (Dobs != 0): min(Dobs, clearance) where
// the field is baked and on, Dobs otherwise.  It does not pass through the collision test (the circles overhang the
// box, so the clearance can be 0 on a state that does not hit).
template <bool LAYERED>
__device__ __forceinline__ double occ_cost_gap(const OccView& ov, int layer, double Dobs, double vpx, double vpy,
                                               double th, double cs, double sn) {
  if (ov.g->field == nullptr || Dobs == 0) return Dobs;
  const double c = occ_clearance<LAYERED>(*ov.g, layer, vpx, vpy, th, cs, sn);
  return c < Dobs ? c : Dobs;
}

}  // namespace clrrt
