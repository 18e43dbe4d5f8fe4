// mjh_ray.h -- ray casting (reference mujoco_torch/_src/ray.py): the primitive intersections the rangefinder sensor shares (mjh_sensor.h) and
// the batched ray kernel behind mjh_ray (ray.py:375-452: ray() with its geom filters, plus the per-triangle mesh test of _ray_mesh / _ray_triangle).
//
// mjh_ray_kernel: one lane per (environment, ray) pair, pairs environment-major, 256 lanes per workgroup.  The candidate geoms (the host's table, in the
// reference's type-major tie-break order) are visited in the same order by every lane, so the type switch and a mesh's triangle loop are wave-uniform and a
// triangle's nine reals are one uniform load for the whole wave.  The candidates' geom_xpos / geom_xmat of the workgroup's environments are staged in LDS
// in chunks of `chunk` candidates (flat loads over (environment, candidate, component): runs of consecutive addresses); the lanes of one environment
// read them from there.  dist / geomid are written at the pair index: one coalesced store each.  First minimum wins (strict <), as torch.argmin.
#pragma once
#include "mjh_device.h"

// world -> geom frame of a ray (ray.py:343-344: x.T @ (pnt - y), x.T @ vec) -- the rangefinder's transform (sensor.py:94-108)
template <typename RT>
__device__ __forceinline__ void ray_to_geom(const RT* gm, const RT* gp, const RT* pnt, const RT* vec, RT* dp, RT* dv) {
  const RT d3[3] = {pnt[0] - gp[0], pnt[1] - gp[1], pnt[2] - gp[2]};
#pragma unroll
  for (int i = 0; i < 3; i++) {
    dp[i] = gm[i] * d3[0] + gm[3 + i] * d3[1] + gm[6 + i] * d3[2];
    dv[i] = gm[i] * vec[0] + gm[3 + i] * vec[1] + gm[6 + i] * vec[2];
  }
}

// RT: the type the intersections run in = the Data dtype (see the header comment)
template <typename RT> __device__ __forceinline__ RT ray_safe_div(RT num, RT den) { return num / (den + (den == 0 ? (RT)(float)mjMINVAL : (RT)0)); }
template <typename RT>
__device__ __forceinline__ void ray_quad(RT a, RT b, RT c, RT& x0, RT& x1) {  // ray.py:28-40
  const RT det = b * b - a * c, det2 = r_sqrt<RT>(det);
  const RT r0 = ray_safe_div<RT>(-b - det2, a), r1 = ray_safe_div<RT>(-b + det2, a);
  const RT inf = (RT)__builtin_inf();
  x0 = ((det < (RT)mjMINVAL) || (r0 < 0)) ? inf : r0;
  x1 = ((det < (RT)mjMINVAL) || (r1 < 0)) ? inf : r1;
}
template <typename RT> __device__ __forceinline__ RT ray_dot3(const RT* a, const RT* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
template <typename RT>
__device__ __forceinline__ RT ray_geom(int type, const RT* size, const RT* pnt, const RT* vec) {
  const RT inf = (RT)__builtin_inf();
  if (type == 0) {  // plane :43-57
    const RT x = -ray_safe_div<RT>(pnt[2], vec[2]);
    bool valid = (vec[2] <= -(RT)mjMINVAL) && (x >= 0);
    for (int i = 0; i < 2; i++) { const RT p = pnt[i] + x * vec[i]; valid = valid && ((size[i] <= 0) || (r_abs(p) <= size[i])); }
    return valid ? x : inf;
  }
  if (type == 2) {  // sphere :60-69
    RT x0, x1;
    ray_quad<RT>(ray_dot3(vec, vec), ray_dot3(vec, pnt), ray_dot3(pnt, pnt) - size[0] * size[0], x0, x1);
    return isinf(x0) ? x1 : x0;
  }
  if (type == 3 || type == 5) {  // capsule :72-106, cylinder :235-268: the round side first
    const RT a = vec[0] * vec[0] + vec[1] * vec[1], b = vec[0] * pnt[0] + vec[1] * pnt[1], c = (pnt[0] * pnt[0] + pnt[1] * pnt[1]) - size[0] * size[0];
    RT x0, x1;
    ray_quad<RT>(a, b, c, x0, x1);
    RT x = isinf(x0) ? x1 : x0;
    x = (r_abs(pnt[2] + x * vec[2]) <= size[1]) ? x : inf;
    for (int cap = 0; cap < 2; cap++) {
      if (type == 3) {  // spherical caps
        const RT dif[3] = {pnt[0], pnt[1], cap == 0 ? pnt[2] - size[1] : pnt[2] + size[1]};
        ray_quad<RT>(ray_dot3(vec, vec), ray_dot3(vec, dif), ray_dot3(dif, dif) - size[0] * size[0], x0, x1);
        if (cap == 0) {
          if ((pnt[2] + x0 * vec[2] >= size[1]) && (x0 < x)) x = x0;
          if ((pnt[2] + x1 * vec[2] >= size[1]) && (x1 < x)) x = x1;
        } else {
          if ((pnt[2] + x0 * vec[2] <= -size[1]) && (x0 < x)) x = x0;
          if ((pnt[2] + x1 * vec[2] <= -size[1]) && (x1 < x)) x = x1;
        }
      } else {  // flat caps
        const RT t = ray_safe_div<RT>((cap == 0 ? size[1] : -size[1]) - pnt[2], vec[2]);
        const RT p0 = pnt[0] + t * vec[0], p1 = pnt[1] + t * vec[1];
        if ((t >= 0) && (p0 * p0 + p1 * p1 <= size[0] * size[0]) && (t < x)) x = t;
      }
    }
    return x;
  }
  if (type == 4) {  // ellipsoid :109-129
    RT s[3], sv[3], sp[3];
    for (int i = 0; i < 3; i++) { s[i] = ray_safe_div<RT>((RT)1, size[i] * size[i]); sv[i] = s[i] * vec[i]; sp[i] = s[i] * pnt[i]; }
    RT x0, x1;
    ray_quad<RT>(ray_dot3(sv, vec), ray_dot3(sv, pnt), ray_dot3(sp, pnt) - 1, x0, x1);
    return isinf(x0) ? x1 : x0;
  }
  if (type == 6) {  // box :132-161
    RT best = inf;
    for (int f = 0; f < 6; f++) {
      const int ax = f % 3, i0 = ax == 0 ? 1 : 0, i1 = ax == 2 ? 1 : 2;
      const RT x = f < 3 ? ray_safe_div<RT>(size[ax] - pnt[ax], vec[ax]) : -ray_safe_div<RT>(size[ax] + pnt[ax], vec[ax]);
      const RT p0 = pnt[i0] + x * vec[i0], p1 = pnt[i1] + x * vec[i1];
      const bool valid = (r_abs(p0) <= size[i0]) && (r_abs(p1) <= size[i1]) && (x >= 0);
      if (valid && x < best) best = x;
    }
    return best;
  }
  return inf;
}

#define MJH_RAY_MESH 7
#define MJH_RAY_WG 256

template <typename REAL>
struct RayArgs {
  const REAL *geom_xpos, *geom_xmat;     // [B, ngeom, 3] / [B, ngeom, 9]
  const REAL *pnt, *vec;                 // ray r of environment e: pnt[e * pnt_env + r * pnt_ray + k] (stride 0: shared)
  int64_t pnt_env, pnt_ray, vec_env, vec_ray;
  const int* cand;                       // [ncand][4]: geom id, geom type, first triangle, end triangle (meshes)
  const REAL* tri;                       // [ntri][9]: triangle vertices in the geom frame
  const REAL* geom_size;                 // [ngeom][3]: the Model's current sizes
  REAL* dist;                            // [B * R]
  int64_t* geomid;                       // [B * R]
  int ngeom, ncand, R;
  int chunk;                             // candidates per LDS chunk
  int64_t env_base;                      // this launch: pairs [env_base * R + r_base, + npairs)
  int r_base, npairs;
};

// distance along the ray to triangle v (9 reals) in the geom frame, with the ray's in-plane basis b, c (ray.py:164-194)
template <typename RT>
__device__ __forceinline__ RT ray_triangle(const RT* v, const RT* pnt, const RT* vec, const RT* b, const RT* c) {
  RT pl[3][2];
#pragma unroll
  for (int i = 0; i < 3; i++) {
    const RT d[3] = {v[3 * i] - pnt[0], v[3 * i + 1] - pnt[1], v[3 * i + 2] - pnt[2]};
    pl[i][0] = d[0] * b[0] + d[1] * b[1] + d[2] * b[2];
    pl[i][1] = d[0] * c[0] + d[1] * c[1] + d[2] * c[2];
  }
  const RT A00 = pl[0][0] - pl[2][0], A01 = pl[0][1] - pl[2][1], A10 = pl[1][0] - pl[2][0], A11 = pl[1][1] - pl[2][1];
  const RT b0 = -pl[2][0], b1 = -pl[2][1];
  const RT det = A00 * A11 - A10 * A01;
  const RT t0 = ray_safe_div<RT>(A11 * b0 - A10 * b1, det), t1 = ray_safe_div<RT>(-A01 * b0 + A00 * b1, det);
  bool valid = (t0 >= 0) && (t1 >= 0) && (t0 + t1 <= 1);
  const RT e0[3] = {v[0] - v[6], v[1] - v[7], v[2] - v[8]}, e1[3] = {v[3] - v[6], v[4] - v[7], v[5] - v[8]};
  const RT n[3] = {e0[1] * e1[2] - e0[2] * e1[1], e0[2] * e1[0] - e0[0] * e1[2], e0[0] * e1[1] - e0[1] * e1[0]};
  const RT w[3] = {v[6] - pnt[0], v[7] - pnt[1], v[8] - pnt[2]};
  const RT dist = ray_safe_div<RT>(w[0] * n[0] + w[1] * n[1] + w[2] * n[2], vec[0] * n[0] + vec[1] * n[1] + vec[2] * n[2]);
  valid = valid && (dist >= 0);
  return valid ? dist : (RT)__builtin_inf();
}

// math.orthogonals(math.normalize(vec)) (math.py:216-243, 485-493): the two in-plane axes of _ray_mesh's basis
template <typename RT>
__device__ __forceinline__ void ray_basis(const RT* vec, RT* b, RT* c) {
  const bool zero = vec[0] == 0 && vec[1] == 0 && vec[2] == 0;
  const RT nv = zero ? (RT)0 : r_sqrt<RT>(vec[0] * vec[0] + vec[1] * vec[1] + vec[2] * vec[2]);
  const RT den = nv + (zero ? (RT)1e-6 : (RT)0);
  const RT a[3] = {vec[0] / den, vec[1] / den, vec[2] / den};
  const bool ydir = ((RT)-0.5 < a[1]) && (a[1] < (RT)0.5);
  const RT y[3] = {(RT)0, ydir ? (RT)1 : (RT)0, ydir ? (RT)0 : (RT)1};
  const RT ab = a[0] * y[0] + a[1] * y[1] + a[2] * y[2];
  RT bb[3] = {y[0] - a[0] * ab, y[1] - a[1] * ab, y[2] - a[2] * ab};
  const bool bzero = bb[0] == 0 && bb[1] == 0 && bb[2] == 0;
  const RT nb = bzero ? (RT)0 : r_sqrt<RT>(bb[0] * bb[0] + bb[1] * bb[1] + bb[2] * bb[2]);
  const RT bden = nb + (bzero ? (RT)1e-6 : (RT)0);
  const RT any = (a[0] != 0 || a[1] != 0 || a[2] != 0) ? (RT)1 : (RT)0;
#pragma unroll
  for (int i = 0; i < 3; i++) b[i] = bb[i] / bden * any;
  c[0] = a[1] * b[2] - a[2] * b[1];
  c[1] = a[2] * b[0] - a[0] * b[2];
  c[2] = a[0] * b[1] - a[1] * b[0];
}

template <typename REAL>
__global__ __launch_bounds__(MJH_RAY_WG) void mjh_ray_kernel(RayArgs<REAL> a) {
  extern __shared__ double ray_lds_raw[];
  REAL* fr = reinterpret_cast<REAL*>(ray_lds_raw);  // [env slot][chunk][12]: geom_xpos (3), geom_xmat (9)
  const int tid = threadIdx.x;
  const unsigned R = (unsigned)a.R;
  const unsigned l0 = blockIdx.x * MJH_RAY_WG, l = l0 + tid;
  const unsigned last = (l0 + MJH_RAY_WG < (unsigned)a.npairs ? l0 + MJH_RAY_WG : (unsigned)a.npairs) - 1;
  const unsigned ef = ((unsigned)a.r_base + l0) / R;              // first environment of the workgroup (relative to env_base)
  const int nenv = (int)(((unsigned)a.r_base + last) / R - ef) + 1;  // environments the workgroup touches
  const bool active = l < (unsigned)a.npairs;
  const unsigned lr = (unsigned)a.r_base + (active ? l : last);
  const unsigned er = lr / R, r = lr - er * R;
  const int slot = (int)(er - ef);
  const int64_t e = a.env_base + er;
  REAL P[3], V[3];
#pragma unroll
  for (int k = 0; k < 3; k++) { P[k] = a.pnt[e * a.pnt_env + r * a.pnt_ray + k]; V[k] = a.vec[e * a.vec_env + r * a.vec_ray + k]; }
  const REAL inf = (REAL)__builtin_inf();
  REAL best = inf;
  int bid = -1;
  const int64_t g0 = (a.env_base + ef) * a.ngeom;  // first geom row of the workgroup's first environment
  for (int c0 = 0; c0 < a.ncand; c0 += a.chunk) {
    const int cn = a.ncand - c0 < a.chunk ? a.ncand - c0 : a.chunk;
    const int n = nenv * cn;  // (environment, candidate) entries of this chunk
    const float inv_cn = 1.0f / (float)cn, inv3 = 1.0f / 3.0f, inv9 = 1.0f / 9.0f;
    __syncthreads();  // (the previous chunk is consumed)
    for (int t = tid; t < 9 * n; t += MJH_RAY_WG) {
      int p, k, s, c;
      split_index(t, 9, inv9, p, k);
      split_index(p, cn, inv_cn, s, c);
      fr[(s * a.chunk + c) * 12 + 3 + k] = a.geom_xmat[(g0 + (int64_t)s * a.ngeom + a.cand[4 * (c0 + c)]) * 9 + k];
    }
    for (int t = tid; t < 3 * n; t += MJH_RAY_WG) {
      int p, k, s, c;
      split_index(t, 3, inv3, p, k);
      split_index(p, cn, inv_cn, s, c);
      fr[(s * a.chunk + c) * 12 + k] = a.geom_xpos[(g0 + (int64_t)s * a.ngeom + a.cand[4 * (c0 + c)]) * 3 + k];
    }
    __syncthreads();
    for (int c = 0; c < cn; c++) {  // wave-uniform: every lane visits the same candidate
      const int* cd = a.cand + 4 * (c0 + c);
      const int g = cd[0], type = cd[1];
      const REAL* f = fr + (slot * a.chunk + c) * 12;
      REAL dp[3], dv[3];
      ray_to_geom<REAL>(f + 3, f, P, V, dp, dv);
      REAL x;
      if (type == MJH_RAY_MESH) {
        REAL bx[3], cx[3];
        ray_basis<REAL>(dv, bx, cx);
        x = inf;
        for (int q = cd[2]; q < cd[3]; q++) {
          const REAL* tv = a.tri + 9 * (int64_t)q;
          REAL v[9];
#pragma unroll
          for (int i = 0; i < 9; i++) v[i] = tv[i];
          const REAL y = ray_triangle<REAL>(v, dp, dv, bx, cx);
          if (y < x) x = y;
        }
      } else {
        const REAL size[3] = {a.geom_size[3 * g], a.geom_size[3 * g + 1], a.geom_size[3 * g + 2]};
        x = ray_geom<REAL>(type, size, dp, dv);
      }
      if (x < best) { best = x; bid = g; }
    }
  }
  if (active) {
    const int64_t o = (int64_t)a.env_base * R + lr;
    a.dist[o] = isinf(best) ? (REAL)-1 : best;
    a.geomid[o] = isinf(best) ? (int64_t)-1 : (int64_t)bid;
  }
}
