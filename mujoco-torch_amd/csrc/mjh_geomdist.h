// mjh_geomdist.h -- signed distance and nearest points of geom pairs on a finished pass (MuJoCo's mj_geomDistance; the reference has no counterpart):
// ONE LANE PER (pair, environment), items PAIR-MAJOR -- consecutive lanes are consecutive environments of the same pair, so the type dispatch below is
// wave-uniform once B >= 64 (a box-box item is a few thousand flops, a sphere-sphere item twenty: environment-major items, as mjh_quadric.h has them, would
// run both under one exec mask).  No LDS, no cross-lane traffic, the 30 reals of an item (two frames, two sizes) loaded up front.
//
// Definitions (n: the unit vector from geom1 towards geom2; to - from = dist * n, overlapping or not):
//  * plane (normal n_p = third column of its frame) against a body: dist = n_p . (c - p) - h, h the body's support height along -n_p (sphere r; capsule
//    r + half |n_l[2]|; box sum size_i |n_l[i]|; ellipsoid |size o n_l|; cylinder r sqrt(n_l[0]^2 + n_l[1]^2) + half |n_l[2]|; n_l = mat^T n_p).  The point on
//    the body is its support point, the point on the plane that point's projection.
//  * sphere, capsule, box = a CORE (point, segment, box: kind 0, 1, 2) plus a radius (r, r, 0): dist = d_core - r1 - r2, the witnesses are the core
//    witnesses moved by the radii along n.  The pair is worked in the frame of the core of the higher kind ("B": the box when there is one), the other ("A")
//    being c, U (centre, axes) there; a core is a box of half-axes h with one (segment) or three (point) of them zero, its corners and edges made from sign
//    bits and h -- never read from an indexed array.
//  * cores that do not overlap: d_core = the minimum over a FIXED enumeration -- every corner of A clamped onto B, every corner of B clamped onto A, every
//    edge of A against every edge of B as segment-segment closest points (box-box: 8 + 8 clamps, 12 x 12 edge pairs).  First minimum wins.
//  * cores that overlap (possible only with a box): the largest signed separation over the face normals of either box and e_a x e_b for every pair of
//    edge directions (a cross product with |e_a x e_b|^2 <= PAR2 is skipped) -- the minimum translation distance; n is that axis.  Whether cores overlap
//    is decided by the sign of that separation.  The witnesses come from the same enumeration, run on A moved out along the axis until the cores touch.
//  * no direction (d_core below TINY times the pair's size): dist stays exact; n is the separation axis when there is a box; else, with a capsule, a unit
//    vector perpendicular to its segment (the cross product of the two axes for capsules whose axes cross, the larger-kind geom's x axis for parallel axes
//    and for a sphere centred on a capsule's axis), so that both points still lie on their surfaces; the world +z for concentric spheres.
// Every loop has a compile-time trip count; nothing iterates to convergence.  Compute is in the Data dtype.
#pragma once
#include "mjh_device.h"

#define MJH_GD_PLANE 0
#define MJH_GD_SPHERE 2
#define MJH_GD_CAPSULE 3
#define MJH_GD_ELLIPSOID 4
#define MJH_GD_CYLINDER 5
#define MJH_GD_BOX 6

template <typename REAL>
struct GeomDistArgs {
  const REAL *geom_xpos, *geom_xmat;  // [B, ngeom, 3] / [B, ngeom, 9]
  const REAL* geom_size;              // [ngeom, 3]: the Model's current sizes
  const int* pairs;                   // [npair][4]: geom1, geom2, type1, type2
  REAL* dist;                         // [B, npair]
  REAL* fromto;                       // [B, npair, 6]
  int64_t B;
  int64_t item_begin, item_count;     // this launch: items [item_begin, item_begin + item_count) of npair * B, item = pair * B + environment
  int ngeom, npair;
  REAL distmax;
};

template <typename REAL> struct GdConst;
template <> struct GdConst<double> { static constexpr double PAR2 = 1e-24, TINY = 1e-13; };
template <> struct GdConst<float> { static constexpr float PAR2 = 1e-10f, TINY = 1e-6f; };

template <typename REAL>
struct GdBest {
  REAL d2, pa[3], pb[3];
  __device__ __forceinline__ void take(REAL c2, const REAL* a, const REAL* b) {  // first minimum wins
    const bool t = c2 < d2;
    d2 = t ? c2 : d2;
#pragma unroll
    for (int i = 0; i < 3; i++) { pa[i] = t ? a[i] : pa[i]; pb[i] = t ? b[i] : pb[i]; }
  }
};

template <typename REAL> __device__ __forceinline__ REAL gd_clamp(REAL x, REAL h) { return r_min(r_max(x, -h), h); }

// local coordinates of corner v of a core of kind K (0: the point, 1: the two ends of the segment along z, 2: the eight corners of the box)
template <int K, typename REAL>
__device__ __forceinline__ void gd_corner(int v, const REAL* h, REAL* s) {
  s[0] = K == 2 ? ((v & 1) ? h[0] : -h[0]) : (REAL)0;
  s[1] = K == 2 ? ((v & 2) ? h[1] : -h[1]) : (REAL)0;
  s[2] = K == 2 ? ((v & 4) ? h[2] : -h[2]) : (K == 1 ? ((v & 1) ? h[2] : -h[2]) : (REAL)0);
}

// the edges of A along its axis JA against the edges of B along its axis IB (B's frame: B's axes are the coordinate axes)
template <int KA, int KB, int JA, int IB, typename REAL>
__device__ __forceinline__ void gd_edges(const REAL* c, const REAL* U, const REAL* a, const REAL* b, GdBest<REAL>& best) {
  constexpr int J1 = (JA + 1) % 3, J2 = (JA + 2) % 3, I1 = (IB + 1) % 3, I2 = (IB + 2) % 3;
  constexpr int NA = KA == 2 ? 4 : 1, NB = KB == 2 ? 4 : 1;
  // u: A's axis JA in B's frame; its part across B's axis IB, (u1, u2), gives sin^2 of the angle between the edges and the unclamped parameter on A's edge,
  // s = -(u1 r1 + u2 r2) / (u1^2 + u2^2), without the cancellation of 1 - (u . e)^2 and (u . e)(e . r) - u . r between nearly parallel edges
  const REAL la = a[JA], lb = b[IB], bb = U[3 * IB + JA], u1 = U[3 * I1 + JA], u2 = U[3 * I2 + JA], denom = u1 * u1 + u2 * u2;
  const bool skew = denom > GdConst<REAL>::PAR2;
  const REAL inv = skew ? (REAL)1 / denom : (REAL)0;
#pragma unroll 1
  for (int k = 0; k < NA * NB; k++) {
    const int ka = k % NA, kb = k / NA;
    REAL ca[3], cb[3] = {0, 0, 0};
    const REAL s1 = KA == 2 ? ((ka & 1) ? a[J1] : -a[J1]) : (REAL)0, s2 = KA == 2 ? ((ka & 2) ? a[J2] : -a[J2]) : (REAL)0;
#pragma unroll
    for (int i = 0; i < 3; i++) ca[i] = c[i] + (U[3 * i + J1] * s1 + U[3 * i + J2] * s2);
    cb[I1] = KB == 2 ? ((kb & 1) ? b[I1] : -b[I1]) : (REAL)0;
    cb[I2] = KB == 2 ? ((kb & 2) ? b[I2] : -b[I2]) : (REAL)0;
    const REAL r[3] = {ca[0] - cb[0], ca[1] - cb[1], ca[2] - cb[2]};
    const REAL cc = U[JA] * r[0] + U[3 + JA] * r[1] + U[6 + JA] * r[2], f = r[IB];
    REAL s = skew ? gd_clamp<REAL>(-(u1 * r[I1] + u2 * r[I2]) * inv, la) : (REAL)0;
    const REAL t = bb * s + f, tc = gd_clamp<REAL>(t, lb);
    s = tc != t ? gd_clamp<REAL>(bb * tc - cc, la) : s;
    REAL pa[3], pb[3] = {cb[0], cb[1], cb[2]};
#pragma unroll
    for (int i = 0; i < 3; i++) pa[i] = ca[i] + U[3 * i + JA] * s;
    pb[IB] = tc;
    const REAL d[3] = {pa[0] - pb[0], pa[1] - pb[1], pa[2] - pb[2]};
    best.take(dot3(d, d), pa, pb);
  }
}

template <int KA, int KB, int JA, typename REAL>
__device__ __forceinline__ void gd_edges_b(const REAL* c, const REAL* U, const REAL* a, const REAL* b, GdBest<REAL>& best) {
  if (KB == 2) { gd_edges<KA, KB, JA, 0>(c, U, a, b, best); gd_edges<KA, KB, JA, 1>(c, U, a, b, best); }
  gd_edges<KA, KB, JA, 2>(c, U, a, b, best);
}

// the fixed enumeration: nearest points of cores A (centre c, axes the columns of U, half-axes a) and B (the coordinate box of half-axes b)
template <int KA, int KB, typename REAL>
__device__ __forceinline__ void gd_enumerate(const REAL* c, const REAL* U, const REAL* a, const REAL* b, GdBest<REAL>& best) {
  constexpr int NVA = KA == 2 ? 8 : (KA == 1 ? 2 : 1), NVB = KB == 2 ? 8 : (KB == 1 ? 2 : 1);
  best.d2 = (REAL)__builtin_inf();
#pragma unroll
  for (int i = 0; i < 3; i++) best.pa[i] = best.pb[i] = 0;
#pragma unroll 1
  for (int v = 0; v < NVA; v++) {  // corners of A onto B
    REAL s[3], p[3], q[3];
    gd_corner<KA, REAL>(v, a, s);
#pragma unroll
    for (int i = 0; i < 3; i++) { p[i] = c[i] + (U[3 * i] * s[0] + U[3 * i + 1] * s[1] + U[3 * i + 2] * s[2]); q[i] = gd_clamp<REAL>(p[i], b[i]); }
    const REAL d[3] = {p[0] - q[0], p[1] - q[1], p[2] - q[2]};
    best.take(dot3(d, d), p, q);
  }
#pragma unroll 1
  for (int v = 0; v < NVB; v++) {  // corners of B onto A
    REAL w[3], z[3], p[3];
    gd_corner<KB, REAL>(v, b, w);
    const REAL r[3] = {w[0] - c[0], w[1] - c[1], w[2] - c[2]};
#pragma unroll
    for (int j = 0; j < 3; j++) z[j] = gd_clamp<REAL>(U[j] * r[0] + U[3 + j] * r[1] + U[6 + j] * r[2], a[j]);
#pragma unroll
    for (int i = 0; i < 3; i++) p[i] = c[i] + (U[3 * i] * z[0] + U[3 * i + 1] * z[1] + U[3 * i + 2] * z[2]);
    const REAL d[3] = {p[0] - w[0], p[1] - w[1], p[2] - w[2]};
    best.take(dot3(d, d), p, w);
  }
  if (KA >= 1 && KB >= 1) {  // edges of A against edges of B
    if (KA == 2) { gd_edges_b<KA, KB, 0>(c, U, a, b, best); gd_edges_b<KA, KB, 1>(c, U, a, b, best); }
    gd_edges_b<KA, KB, 2>(c, U, a, b, best);
  }
}

// one candidate separation axis d (unit, B's frame): the signed separation of the cores along it; the largest wins, first on a tie
template <typename REAL>
__device__ __forceinline__ void gd_axis(const REAL* d, const REAL* c, const REAL* U, const REAL* a, const REAL* b, REAL& sep, REAL* n) {
  const REAL cd = dot3(c, d);
  REAL reach = 0;
#pragma unroll
  for (int j = 0; j < 3; j++) reach += a[j] * r_abs<REAL>(U[j] * d[0] + U[3 + j] * d[1] + U[6 + j] * d[2]) + b[j] * r_abs<REAL>(d[j]);
  const REAL s = r_abs<REAL>(cd) - reach;
  const bool t = s > sep;
  sep = t ? s : sep;
#pragma unroll
  for (int i = 0; i < 3; i++) n[i] = t ? (cd > 0 ? -d[i] : d[i]) : n[i];  // from A (at c) towards B (at the origin)
}

// the largest signed separation of core A from the box B over the face normals and the edge cross products: sep, and its axis n from A towards B
template <int KA, typename REAL>
__device__ __forceinline__ void gd_separation(const REAL* c, const REAL* U, const REAL* a, const REAL* b, REAL& sep, REAL* n) {
  sep = -(REAL)__builtin_inf();
  n[0] = n[1] = 0; n[2] = 1;
#pragma unroll
  for (int i = 0; i < 3; i++) {
    const REAL d[3] = {(REAL)(i == 0), (REAL)(i == 1), (REAL)(i == 2)};
    gd_axis<REAL>(d, c, U, a, b, sep, n);
  }
  if (KA == 2) {
#pragma unroll
    for (int j = 0; j < 3; j++) {
      const REAL d[3] = {U[j], U[3 + j], U[6 + j]};
      gd_axis<REAL>(d, c, U, a, b, sep, n);
    }
  }
  if (KA >= 1) {
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
      for (int j = (KA == 2 ? 0 : 2); j < 3; j++) {
        const REAL e[3] = {(REAL)(i == 0), (REAL)(i == 1), (REAL)(i == 2)}, u[3] = {U[j], U[3 + j], U[6 + j]};
        REAL m[3];
        cross3(e, u, m);
        const REAL m2 = dot3(m, m);
        if (m2 > GdConst<REAL>::PAR2) {
          const REAL inv = (REAL)1 / r_sqrt<REAL>(m2);
          const REAL d[3] = {m[0] * inv, m[1] * inv, m[2] * inv};
          gd_axis<REAL>(d, c, U, a, b, sep, n);
        }
      }
    }
  }
}

// cores of kinds KA <= KB with radii ra, rb: A = (pa_w, ma, ha), B = (pb_w, mb, hb) in the world; writes the signed distance and the two surface points (world)
template <int KA, int KB, typename REAL>
__device__ __forceinline__ REAL gd_cores(const REAL* pa_w, const REAL* ma, const REAL* ha, REAL ra, const REAL* pb_w, const REAL* mb, const REAL* hb, REAL rb,
                                         REAL* on_a, REAL* on_b) {
  REAL c[3], U[9];
  const REAL rel[3] = {pa_w[0] - pb_w[0], pa_w[1] - pb_w[1], pa_w[2] - pb_w[2]};
#pragma unroll
  for (int i = 0; i < 3; i++) {
    c[i] = mb[i] * rel[0] + mb[3 + i] * rel[1] + mb[6 + i] * rel[2];
#pragma unroll
    for (int j = 0; j < 3; j++) U[3 * i + j] = mb[i] * ma[j] + mb[3 + i] * ma[3 + j] + mb[6 + i] * ma[6 + j];
  }
  // the direction where the cores leave none: the world +z (in B's frame) for two points; with a segment, a unit vector perpendicular to it -- B's x axis, or
  // for two segments the cross product of the axes unless they are parallel --, so that a point moved by a radius along it stays on the capsule's surface
  REAL sep = 1, n[3] = {mb[6], mb[7], mb[8]};
  if (KB == 1) {
    n[0] = 1; n[1] = 0; n[2] = 0;
    if (KA == 1) {  // (U[2], U[5], U[8]) x e_z
      const REAL m2 = U[2] * U[2] + U[5] * U[5];
      if (m2 > GdConst<REAL>::PAR2) {
        const REAL inv = (REAL)1 / r_sqrt<REAL>(m2);
        n[0] = U[5] * inv; n[1] = -U[2] * inv;
      }
    }
  }
  if (KB == 2) gd_separation<KA, REAL>(c, U, ha, hb, sep, n);
  const bool overlap = KB == 2 && sep <= 0;
  REAL cs[3];
#pragma unroll
  for (int i = 0; i < 3; i++) cs[i] = overlap ? c[i] + sep * n[i] : c[i];  // overlapping cores: A moved out along the axis until they touch
  GdBest<REAL> best;
  gd_enumerate<KA, KB, REAL>(cs, U, ha, hb, best);
  REAL dcore, qa[3], qb[3];
  if (overlap) {
    dcore = sep;
#pragma unroll
    for (int i = 0; i < 3; i++) { qb[i] = best.pb[i]; qa[i] = best.pb[i] - sep * n[i]; }
  } else {
    dcore = r_sqrt<REAL>(best.d2);
    const REAL size = ra + rb + ha[0] + ha[1] + ha[2] + hb[0] + hb[1] + hb[2];
    const bool dir = dcore > GdConst<REAL>::TINY * size;
    const REAL inv = dir ? (REAL)1 / dcore : (REAL)0;
#pragma unroll
    for (int i = 0; i < 3; i++) { qa[i] = best.pa[i]; qb[i] = best.pb[i]; n[i] = dir ? (qb[i] - qa[i]) * inv : n[i]; }
  }
#pragma unroll
  for (int i = 0; i < 3; i++) { qa[i] = qa[i] + ra * n[i]; qb[i] = qb[i] - rb * n[i]; }
#pragma unroll
  for (int i = 0; i < 3; i++) {
    on_a[i] = pb_w[i] + (mb[3 * i] * qa[0] + mb[3 * i + 1] * qa[1] + mb[3 * i + 2] * qa[2]);
    on_b[i] = pb_w[i] + (mb[3 * i] * qb[0] + mb[3 * i + 1] * qb[1] + mb[3 * i + 2] * qb[2]);
  }
  return dcore - ra - rb;
}

// plane (point pp, normal np) against a body of type `type`: the signed distance, the body's support point and its projection onto the plane
template <typename REAL>
__device__ __forceinline__ REAL gd_plane(const REAL* pp, const REAL* np, int type, const REAL* c, const REAL* m, const REAL* size, REAL* on_plane, REAL* on_body) {
  REAL nl[3], s[3] = {0, 0, 0}, rad = 0;  // the support point along -np: c + m s - rad np
#pragma unroll
  for (int i = 0; i < 3; i++) nl[i] = m[i] * np[0] + m[3 + i] * np[1] + m[6 + i] * np[2];
  if (type == MJH_GD_SPHERE) {
    rad = size[0];
  } else if (type == MJH_GD_CAPSULE) {
    rad = size[0];
    s[2] = nl[2] < 0 ? size[1] : -size[1];
  } else if (type == MJH_GD_BOX) {
#pragma unroll
    for (int i = 0; i < 3; i++) s[i] = nl[i] < 0 ? size[i] : -size[i];
  } else if (type == MJH_GD_ELLIPSOID) {
    const REAL v[3] = {size[0] * nl[0], size[1] * nl[1], size[2] * nl[2]};
    const REAL len = r_sqrt<REAL>(dot3(v, v)), inv = len > 0 ? (REAL)1 / len : (REAL)0;
#pragma unroll
    for (int i = 0; i < 3; i++) s[i] = -size[i] * v[i] * inv;
  } else {  // MJH_GD_CYLINDER
    const REAL len = r_sqrt<REAL>(nl[0] * nl[0] + nl[1] * nl[1]), inv = len > 0 ? size[0] / len : (REAL)0;  // (the disc flat on the plane: its centre)
    s[0] = -nl[0] * inv; s[1] = -nl[1] * inv;
    s[2] = nl[2] < 0 ? size[1] : -size[1];
  }
#pragma unroll
  for (int i = 0; i < 3; i++) on_body[i] = c[i] + (m[3 * i] * s[0] + m[3 * i + 1] * s[1] + m[3 * i + 2] * s[2]) - rad * np[i];
  const REAL rel[3] = {on_body[0] - pp[0], on_body[1] - pp[1], on_body[2] - pp[2]};
  const REAL dist = dot3(np, rel);
#pragma unroll
  for (int i = 0; i < 3; i++) on_plane[i] = on_body[i] - dist * np[i];
  return dist;
}

template <typename REAL> __device__ __forceinline__ int gd_kind(int type) { return type == MJH_GD_SPHERE ? 0 : (type == MJH_GD_CAPSULE ? 1 : (type == MJH_GD_BOX ? 2 : -1)); }

// grid: ceil(item_count / 64) one-wave workgroups; no grid-stride loop
template <typename REAL>
__global__ __launch_bounds__(MJH_WAVE) void mjh_geomdist_kernel(GeomDistArgs<REAL> a) {
  const int64_t local = (int64_t)blockIdx.x * MJH_WAVE + threadIdx.x;
  if (local >= a.item_count) return;
  const int64_t item = a.item_begin + local;
  const int p = (int)(item / a.B);
  const int64_t e = item - (int64_t)p * a.B;
  const int g1 = a.pairs[4 * p], g2 = a.pairs[4 * p + 1], t1 = a.pairs[4 * p + 2], t2 = a.pairs[4 * p + 3];
  const int64_t o = e * a.npair + p;
  const REAL nan = (REAL)__builtin_nan("");
  REAL dist = nan, from[3] = {nan, nan, nan}, to[3] = {nan, nan, nan};
  if ((unsigned)g1 < (unsigned)a.ngeom && (unsigned)g2 < (unsigned)a.ngeom) {  // (the host validates the table; a bad row reads nothing)
    REAL p1[3], p2[3], m1[9], m2[9], s1[3], s2[3];
    const REAL *gp = a.geom_xpos + e * a.ngeom * 3, *gm = a.geom_xmat + e * a.ngeom * 9;
#pragma unroll
    for (int i = 0; i < 3; i++) { p1[i] = gp[3 * g1 + i]; p2[i] = gp[3 * g2 + i]; s1[i] = a.geom_size[3 * g1 + i]; s2[i] = a.geom_size[3 * g2 + i]; }
#pragma unroll
    for (int i = 0; i < 9; i++) { m1[i] = gm[9 * g1 + i]; m2[i] = gm[9 * g2 + i]; }
    const int k1 = gd_kind<REAL>(t1), k2 = gd_kind<REAL>(t2);
    if (t1 == MJH_GD_PLANE && t2 != MJH_GD_PLANE && (k2 >= 0 || t2 == MJH_GD_ELLIPSOID || t2 == MJH_GD_CYLINDER)) {
      const REAL np[3] = {m1[2], m1[5], m1[8]};
      dist = gd_plane<REAL>(p1, np, t2, p2, m2, s2, from, to);
    } else if (t2 == MJH_GD_PLANE && t1 != MJH_GD_PLANE && (k1 >= 0 || t1 == MJH_GD_ELLIPSOID || t1 == MJH_GD_CYLINDER)) {
      const REAL np[3] = {m2[2], m2[5], m2[8]};
      dist = gd_plane<REAL>(p2, np, t1, p1, m1, s1, to, from);
    } else if (k1 >= 0 && k2 >= 0) {
      // A: the core of the lower kind, B: of the higher (geom1 on a tie); half-axes with the zeros of the point and the segment written out
      const bool swap = k1 > k2;
      const int ka = swap ? k2 : k1, kb = swap ? k1 : k2;
      REAL pa[3], pb[3], ma[9], mb[9], ha[3], hb[3], on_a[3], on_b[3];
#pragma unroll
      for (int i = 0; i < 3; i++) { pa[i] = swap ? p2[i] : p1[i]; pb[i] = swap ? p1[i] : p2[i]; }
#pragma unroll
      for (int i = 0; i < 9; i++) { ma[i] = swap ? m2[i] : m1[i]; mb[i] = swap ? m1[i] : m2[i]; }
      const REAL sa0 = swap ? s2[0] : s1[0], sa1 = swap ? s2[1] : s1[1], sa2 = swap ? s2[2] : s1[2];
      const REAL sb0 = swap ? s1[0] : s2[0], sb1 = swap ? s1[1] : s2[1], sb2 = swap ? s1[2] : s2[2];
      const REAL ra = ka == 2 ? (REAL)0 : sa0, rb = kb == 2 ? (REAL)0 : sb0;
      ha[0] = ka == 2 ? sa0 : (REAL)0; ha[1] = ka == 2 ? sa1 : (REAL)0; ha[2] = ka == 2 ? sa2 : (ka == 1 ? sa1 : (REAL)0);
      hb[0] = kb == 2 ? sb0 : (REAL)0; hb[1] = kb == 2 ? sb1 : (REAL)0; hb[2] = kb == 2 ? sb2 : (kb == 1 ? sb1 : (REAL)0);
      if (kb == 0) dist = gd_cores<0, 0, REAL>(pa, ma, ha, ra, pb, mb, hb, rb, on_a, on_b);
      else if (kb == 1) dist = ka == 0 ? gd_cores<0, 1, REAL>(pa, ma, ha, ra, pb, mb, hb, rb, on_a, on_b) : gd_cores<1, 1, REAL>(pa, ma, ha, ra, pb, mb, hb, rb, on_a, on_b);
      else if (ka == 0) dist = gd_cores<0, 2, REAL>(pa, ma, ha, ra, pb, mb, hb, rb, on_a, on_b);
      else if (ka == 1) dist = gd_cores<1, 2, REAL>(pa, ma, ha, ra, pb, mb, hb, rb, on_a, on_b);
      else dist = gd_cores<2, 2, REAL>(pa, ma, ha, ra, pb, mb, hb, rb, on_a, on_b);
#pragma unroll
      for (int i = 0; i < 3; i++) { from[i] = swap ? on_b[i] : on_a[i]; to[i] = swap ? on_a[i] : on_b[i]; }
    }
  }
  const bool cut = dist > a.distmax;  // MuJoCo's convention beyond distmax
  a.dist[o] = cut ? a.distmax : dist;
#pragma unroll
  for (int i = 0; i < 3; i++) { a.fromto[o * 6 + i] = cut ? (REAL)0 : from[i]; a.fromto[o * 6 + 3 + i] = cut ? (REAL)0 : to[i]; }
}
