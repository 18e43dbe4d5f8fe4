// mjh_render.h -- the ray-cast renderer behind mjh_render (reference mujoco_torch/_src/render.py: render / render_batch).
//
// mjh_render_kernel: one lane per (environment, output pixel), pixels environment-major (row-major within an image), 256 lanes per workgroup, so a
// workgroup touches one or two environments (more only for images under 256 pixels).  Per lane and per super-sample: the pixel's primary ray
// (_generate_rays), its nearest hit among the candidate geoms (ray_precomputed + _intersect_meshes: the primitives in the reference's type-major
// order, first minimum wins, then the meshes triangle by triangle, a mesh winning only when strictly closer), the hit geom's colour (_geom_color),
// its shading (_compute_normals, _shade: Lambert + Phong per light, attenuation, spotlight cone, shadow rays against the primitives) and fog
// (_apply_fog).  The super-samples of an output pixel are averaged in registers: the large image is never written.
//
// The candidates' geom_xpos / geom_xmat of the workgroup's environments are staged in LDS as mjh_ray_kernel does; when they do not fit in one
// chunk, every pass over the candidates (the primary ray, each shadow ray) re-stages them chunk by chunk -- every lane runs the same passes, so the
// barriers are uniform.  The candidate loops are wave-uniform; camera and light poses are per-environment loads (one or two distinct addresses
// per wave).  The primary hit is the arithmetic of mjh_ray_kernel (ray_to_geom, ray_geom, ray_basis, ray_triangle) on the same ray.
//
// Dtypes follow the reference: MuJoCo keeps geom_rgba / mat_rgba / the light colours in float32, so the products base colour x light colour and
// the flat colour are float32 values even in a float64 model; everything else runs in the model dtype.  `rgb_f32` writes rgb as float32 (the
// reference's flat, unfogged image), `u8` writes (rgb * 255).clamp(0, 255) truncated to uint8 from the rgb of that dtype.
#pragma once
#include "mjh_device.h"
#include "mjh_ray.h"

#define MJH_RENDER_WG 256
#define MJH_RENDER_LIGHT 16  // reals per light row (include/mjhip.h mjhRenderScene)

template <typename REAL>
struct RenderArgs {
  const REAL *geom_xpos, *geom_xmat;    // [B, ngeom, 3] / [B, ngeom, 9]
  const REAL *cam_xpos, *cam_xmat;      // [B, ncam, 3] / [B, ncam, 9]
  const REAL *light_xpos, *light_xdir;  // [B, nlight, 3]
  const int* cand;                      // [ncand][4]: geom id, geom type, first / end triangle (meshes); primitives first
  const REAL* tri;                      // [ntri][9]
  const REAL* geom_size;                // [ngeom][3]
  const REAL* geom_rgba;                // [ngeom][4] (float32 values)
  const int* geom_matid;                // [ngeom]
  const float* mat_rgba;                // [nmat][4]
  const REAL* light;                    // [nlight][MJH_RENDER_LIGHT]
  void* rgb;                            // [B * P * 3]: REAL, float or uint8
  REAL* depth;                          // [B * P]
  int64_t* seg;                         // [B * P]
  REAL half_w, half_h, fog_start, fog_range, fog_color[3];
  float bg[3];
  int ngeom, ncam, nlight, cam, ncand, nprim, chunk;
  int W, H, ssaa;                       // output size, super-sampling factor
  int shade, shadows, fog, rgb_f32, u8;
  int64_t env_base;                     // this launch: pairs [env_base * P + r_base, + npairs)
  int r_base, npairs;
};

template <typename RT> __device__ __forceinline__ RT rnd_norm3(const RT* v) { return r_sqrt<RT>(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]); }
template <typename RT> __device__ __forceinline__ RT rnd_sign(RT x) { return x > 0 ? (RT)1 : (x < 0 ? (RT)-1 : (RT)0); }
// render.py:387-389 _safe_normalize: v / max(|v|, 1e-10)
template <typename RT>
__device__ __forceinline__ void rnd_safe_normalize(RT* v) {
  RT n = rnd_norm3<RT>(v);
  n = n < (RT)1e-10 ? (RT)1e-10 : n;
  v[0] = v[0] / n; v[1] = v[1] / n; v[2] = v[2] / n;
}

// the candidates' frames of the workgroup's environments (environment slots [0, nenv)), candidates [c0, c0 + cn), into fr[(slot * chunk + c) * 12]
template <typename REAL>
__device__ __forceinline__ void rnd_stage(const RenderArgs<REAL>& a, REAL* fr, int64_t g0, int nenv, int c0, int cn, int tid) {
  const int n = nenv * cn;
  const float inv_cn = 1.0f / (float)cn, inv3 = 1.0f / 3.0f, inv9 = 1.0f / 9.0f;
  for (int t = tid; t < 9 * n; t += MJH_RENDER_WG) {
    int p, k, s, c;
    split_index(t, 9, inv9, p, k);
    split_index(p, cn, inv_cn, s, c);
    fr[(s * a.chunk + c) * 12 + 3 + k] = a.geom_xmat[(g0 + (int64_t)s * a.ngeom + a.cand[4 * (c0 + c)]) * 9 + k];
  }
  for (int t = tid; t < 3 * n; t += MJH_RENDER_WG) {
    int p, k, s, c;
    split_index(t, 3, inv3, p, k);
    split_index(p, cn, inv_cn, s, c);
    fr[(s * a.chunk + c) * 12 + k] = a.geom_xpos[(g0 + (int64_t)s * a.ngeom + a.cand[4 * (c0 + c)]) * 3 + k];
  }
}

// nearest hit of ray (P, V) over candidates [0, nc) (`meshes`: the mesh rows too, the primary ray; else the primitives only, a shadow ray).
// Every lane of the workgroup calls it the same number of times (its barriers).  Returns the distance (inf: none) and the candidate row in `bc`.
template <typename REAL>
__device__ __forceinline__ REAL rnd_nearest(const RenderArgs<REAL>& a, REAL* fr, bool resident, int64_t g0, int nenv, int slot, int tid, const REAL* P,
                                            const REAL* V, int nc, bool meshes, int& bc) {
  const REAL inf = (REAL)__builtin_inf();
  REAL best = inf;
  bc = -1;
  for (int c0 = 0; c0 < nc; c0 += a.chunk) {
    const int cn = nc - c0 < a.chunk ? nc - c0 : a.chunk;
    if (!resident) {
      __syncthreads();  // (the previous chunk is consumed)
      rnd_stage<REAL>(a, fr, g0, nenv, c0, cn, tid);
      __syncthreads();
    }
    for (int c = 0; c < cn; c++) {  // wave-uniform
      const int* cd = a.cand + 4 * (c0 + c);
      const int g = cd[0], type = cd[1];
      const REAL* f = fr + (slot * a.chunk + c) * 12;
      REAL dp[3], dv[3];
      ray_to_geom<REAL>(f + 3, f, P, V, dp, dv);
      if (type == MJH_RAY_MESH) {
        if (!meshes) continue;
        REAL bx[3], cx[3];
        ray_basis<REAL>(dv, bx, cx);
        REAL x = inf;
        for (int q = cd[2]; q < cd[3]; q++) {
          const REAL* tv = a.tri + 9 * (int64_t)q;
          REAL v[9];
#pragma unroll
          for (int i = 0; i < 9; i++) v[i] = tv[i];
          const REAL y = ray_triangle<REAL>(v, dp, dv, bx, cx);
          if (y < x) x = y;
        }
        if (x > 0 && x < best) { best = x; bc = c0 + c; }  // render.py:676-677: a mesh replaces a hit only when strictly closer, at a positive distance
      } else {
        const REAL size[3] = {a.geom_size[3 * g], a.geom_size[3 * g + 1], a.geom_size[3 * g + 2]};
        const REAL x = ray_geom<REAL>(type, size, dp, dv);
        if (x < best) { best = x; bc = c0 + c; }
      }
    }
  }
  return best;
}

// world-frame normal at hit point `hit` of geom g of type `type` in environment e (render.py:392-476)
template <typename REAL>
__device__ __forceinline__ void rnd_normal(const RenderArgs<REAL>& a, int64_t e, int g, int type, const REAL* hit, REAL* nw) {
  const REAL* gp = a.geom_xpos + (e * a.ngeom + g) * 3;
  const REAL* gm = a.geom_xmat + (e * a.ngeom + g) * 9;
  REAL xp[3], xm[9];
#pragma unroll
  for (int i = 0; i < 3; i++) xp[i] = gp[i];
#pragma unroll
  for (int i = 0; i < 9; i++) xm[i] = gm[i];
  const REAL d3[3] = {hit[0] - xp[0], hit[1] - xp[1], hit[2] - xp[2]};
  REAL hl[3];
#pragma unroll
  for (int i = 0; i < 3; i++) hl[i] = xm[i] * d3[0] + xm[3 + i] * d3[1] + xm[6 + i] * d3[2];
  const REAL s0 = a.geom_size[3 * g], s1 = a.geom_size[3 * g + 1], s2 = a.geom_size[3 * g + 2];
  REAL n[3] = {(REAL)0, (REAL)0, (REAL)1};  // plane
  if (type == 2 || type == MJH_RAY_MESH) {  // sphere; mesh: the reference's radial approximation
    n[0] = hl[0]; n[1] = hl[1]; n[2] = hl[2];
    rnd_safe_normalize<REAL>(n);
  } else if (type == 4) {  // ellipsoid
    const REAL q[3] = {s0 * s0, s1 * s1, s2 * s2};
    for (int i = 0; i < 3; i++) n[i] = hl[i] / (q[i] < (REAL)1e-10 ? (REAL)1e-10 : q[i]);
    rnd_safe_normalize<REAL>(n);
  } else if (type == 6) {  // box: the face of the largest |hl| / size (first on a tie, as argmax)
    const REAL sz[3] = {s0 < (REAL)1e-10 ? (REAL)1e-10 : s0, s1 < (REAL)1e-10 ? (REAL)1e-10 : s1, s2 < (REAL)1e-10 ? (REAL)1e-10 : s2};
    const REAL q0 = r_abs(hl[0]) / sz[0], q1 = r_abs(hl[1]) / sz[1], q2 = r_abs(hl[2]) / sz[2];
    const int f = (q1 > q0) ? ((q2 > q1) ? 2 : 1) : ((q2 > q0) ? 2 : 0);
    n[2] = (REAL)0;
    n[0] = f == 0 ? rnd_sign<REAL>(hl[0]) : (REAL)0;
    n[1] = f == 1 ? rnd_sign<REAL>(hl[1]) : (REAL)0;
    n[2] = f == 2 ? rnd_sign<REAL>(hl[2]) : (REAL)0;
  } else if (type == 3 || type == 5) {  // capsule: spherical cap or round side; cylinder: flat cap or round side
    const bool cap = type == 3 ? r_abs(hl[2]) > s1 : r_abs(hl[2]) > (s1 - (REAL)1e-6);
    if (cap && type == 3) {
      n[0] = hl[0]; n[1] = hl[1]; n[2] = hl[2] - rnd_sign<REAL>(hl[2]) * s1;
      rnd_safe_normalize<REAL>(n);
    } else if (cap) {
      n[0] = (REAL)0; n[1] = (REAL)0; n[2] = rnd_sign<REAL>(hl[2]);
    } else {
      REAL r = r_sqrt<REAL>(hl[0] * hl[0] + hl[1] * hl[1]);
      r = r < (REAL)1e-10 ? (REAL)1e-10 : r;
      n[0] = hl[0] / r; n[1] = hl[1] / r; n[2] = (REAL)0;
    }
  }
#pragma unroll
  for (int i = 0; i < 3; i++) nw[i] = xm[3 * i] * n[0] + xm[3 * i + 1] * n[1] + xm[3 * i + 2] * n[2];
}

template <typename REAL>
__global__ __launch_bounds__(MJH_RENDER_WG) void mjh_render_kernel(RenderArgs<REAL> a) {
  extern __shared__ double rnd_lds_raw[];
  REAL* fr = reinterpret_cast<REAL*>(rnd_lds_raw);  // [env slot][chunk][12]: geom_xpos (3), geom_xmat (9)
  const int tid = threadIdx.x;
  const unsigned P = (unsigned)(a.W * a.H);
  const unsigned l0 = blockIdx.x * MJH_RENDER_WG, l = l0 + tid;
  const unsigned last = (l0 + MJH_RENDER_WG < (unsigned)a.npairs ? l0 + MJH_RENDER_WG : (unsigned)a.npairs) - 1;
  const unsigned ef = ((unsigned)a.r_base + l0) / P;               // first environment of the workgroup (relative to env_base)
  const int nenv = (int)(((unsigned)a.r_base + last) / P - ef) + 1;  // environments the workgroup touches
  const bool active = l < (unsigned)a.npairs;
  const unsigned lr = (unsigned)a.r_base + (active ? l : last);
  const unsigned er = lr / P, r = lr - er * P;
  const int slot = (int)(er - ef);
  const int64_t e = a.env_base + er;
  const int64_t g0 = (a.env_base + ef) * a.ngeom;
  const bool resident = a.chunk >= a.ncand;
  if (resident && a.ncand > 0) {
    rnd_stage<REAL>(a, fr, g0, nenv, 0, a.ncand, tid);
    __syncthreads();
  }
  const int py = (int)(r / (unsigned)a.W), px = (int)(r - (unsigned)py * (unsigned)a.W);
  const int S = a.ssaa, RW = a.W * S, RH = a.H * S;
  REAL cp[3], cm[9];
#pragma unroll
  for (int i = 0; i < 3; i++) cp[i] = a.cam_xpos[(e * a.ncam + a.cam) * 3 + i];
#pragma unroll
  for (int i = 0; i < 9; i++) cm[i] = a.cam_xmat[(e * a.ncam + a.cam) * 9 + i];
  const REAL inf = (REAL)__builtin_inf();
  REAL acc[3] = {(REAL)0, (REAL)0, (REAL)0}, dacc = (REAL)0;
  int64_t segv = -1;
  for (int sy = 0; sy < S; sy++) {
    for (int sx = 0; sx < S; sx++) {
      // render.py:179-217: pixel centre u, v; camera-frame direction, normalised, rotated by cam_xmat
      const REAL u = (REAL)(px * S + sx) + (REAL)0.5, v = (REAL)(py * S + sy) + (REAL)0.5;
      REAL dc[3] = {((REAL)2 * u / (REAL)RW - (REAL)1) * a.half_w, ((REAL)1 - (REAL)2 * v / (REAL)RH) * a.half_h, (REAL)-1};
      const REAL dn = rnd_norm3<REAL>(dc);
      dc[0] = dc[0] / dn; dc[1] = dc[1] / dn; dc[2] = dc[2] / dn;
      REAL V[3];
#pragma unroll
      for (int i = 0; i < 3; i++) V[i] = cm[3 * i] * dc[0] + cm[3 * i + 1] * dc[1] + cm[3 * i + 2] * dc[2];
      int bc;
      const REAL best = rnd_nearest<REAL>(a, fr, resident, g0, nenv, slot, tid, cp, V, a.ncand, true, bc);
      const bool hit = best < inf;
      const REAL depth = hit ? best : (REAL)-1;
      const int g = hit ? a.cand[4 * bc] : -1;
      if (sy == S / 2 && sx == S / 2) segv = g;
      // render.py:225-246 _geom_color: the material's rgba, else the geom's (float32 values)
      float base[3] = {0.f, 0.f, 0.f};
      if (hit) {
        const int mid = a.geom_matid[g];
#pragma unroll
        for (int k = 0; k < 3; k++) base[k] = mid >= 0 ? a.mat_rgba[4 * mid + k] : (float)a.geom_rgba[4 * g + k];
      }
      REAL col[3] = {(REAL)base[0], (REAL)base[1], (REAL)base[2]};
      if (a.shade) {  // render.py:522-624 _shade
        const REAL hp[3] = {cp[0] + best * V[0], cp[1] + best * V[1], cp[2] + best * V[2]};
        REAL nw[3] = {(REAL)0, (REAL)0, (REAL)0};
        if (hit) rnd_normal<REAL>(a, e, g, a.cand[4 * bc + 1], hp, nw);
        REAL sh[3] = {(REAL)0, (REAL)0, (REAL)0};
        for (int li = 0; li < a.nlight; li++) {
          const REAL* L = a.light + MJH_RENDER_LIGHT * li;
          const bool directional = L[13] != 0;
          const REAL* lp = a.light_xpos + (e * a.nlight + li) * 3;
          const REAL* ld = a.light_xdir + (e * a.nlight + li) * 3;
          const REAL ldir[3] = {ld[0], ld[1], ld[2]};
          REAL tl[3];
          if (directional) { tl[0] = -ldir[0]; tl[1] = -ldir[1]; tl[2] = -ldir[2]; }
          else { tl[0] = lp[0] - hp[0]; tl[1] = lp[1] - hp[1]; tl[2] = lp[2] - hp[2]; }
          const REAL dist = rnd_norm3<REAL>(tl);
          rnd_safe_normalize<REAL>(tl);
          REAL att = (REAL)1;
          if (!directional) {
            REAL q = L[9] + L[10] * dist + L[11] * dist * dist;
            q = q < (REAL)1e-10 ? (REAL)1e-10 : q;
            att = (REAL)1 / q;
          }
          REAL spot = (REAL)1;
          if (L[12] <= (REAL)1) {  // cutoff < 180 degrees: cos^10 inside the cone (the reference ignores light_exponent)
            REAL sd[3] = {ldir[0], ldir[1], ldir[2]};
            rnd_safe_normalize<REAL>(sd);
            const REAL ca = -tl[0] * sd[0] + -tl[1] * sd[1] + -tl[2] * sd[2];
            spot = ca > L[12] ? pow(ca < 0 ? (REAL)0 : ca, (REAL)10) : (REAL)0;
          }
          bool shadowed = false;
          if (a.shadows && L[14] != 0) {  // render.py:484-514: a ray toward the light from just off the surface, against the primitives
            const REAL eps = (REAL)1e-4;
            const REAL so[3] = {hp[0] + tl[0] * eps, hp[1] + tl[1] * eps, hp[2] + tl[2] * eps};
            int sc;
            const REAL sdist = rnd_nearest<REAL>(a, fr, resident, g0, nenv, slot, tid, so, tl, a.nprim, false, sc);
            const REAL lim = directional ? inf : dist;
            shadowed = sdist < inf && sdist > 0 && sdist < lim - (REAL)2 * eps;
          }
          REAL ndl = nw[0] * tl[0] + nw[1] * tl[1] + nw[2] * tl[2];
          ndl = ndl < 0 ? (REAL)0 : ndl;
          REAL rf[3] = {(REAL)2 * ndl * nw[0] - tl[0], (REAL)2 * ndl * nw[1] - tl[1], (REAL)2 * ndl * nw[2] - tl[2]};
          rnd_safe_normalize<REAL>(rf);
          REAL rdv = -V[0] * rf[0] + -V[1] * rf[1] + -V[2] * rf[2];
          rdv = rdv < 0 ? (REAL)0 : rdv;
          const REAL p50 = pow(rdv, (REAL)50);
#pragma unroll
          for (int k = 0; k < 3; k++) {
            const REAL amb = (REAL)(base[k] * (float)L[3 + k]);  // float32 x float32 (render.py:610)
            const REAL dif = (REAL)(base[k] * (float)L[k]) * ndl;
            const REAL spe = L[6 + k] * p50;
            sh[k] = sh[k] + (shadowed ? amb : amb + (dif + spe) * att * spot);
          }
        }
#pragma unroll
        for (int k = 0; k < 3; k++) col[k] = sh[k] < 0 ? (REAL)0 : (sh[k] > 1 ? (REAL)1 : sh[k]);
      }
      if (!hit) { col[0] = (REAL)a.bg[0]; col[1] = (REAL)a.bg[1]; col[2] = (REAL)a.bg[2]; }
      if (a.fog) {  // render.py:693-711, on hit samples only
        REAL f = ((depth < 0 ? (REAL)0 : depth) - a.fog_start) / a.fog_range;
        f = f < 0 ? (REAL)0 : (f > 1 ? (REAL)1 : f);
        f = depth < 0 ? (REAL)0 : f;
#pragma unroll
        for (int k = 0; k < 3; k++) col[k] = col[k] * ((REAL)1 - f) + a.fog_color[k] * f;
      }
#pragma unroll
      for (int k = 0; k < 3; k++) acc[k] = acc[k] + col[k];
      dacc = dacc + depth;
    }
  }
  if (active) {
    const int64_t o = (int64_t)a.env_base * P + lr;
    const REAL ns = (REAL)(S * S);
    REAL c[3] = {acc[0], acc[1], acc[2]};
    REAL dep = dacc;
    if (S > 1) { c[0] = c[0] / ns; c[1] = c[1] / ns; c[2] = c[2] / ns; dep = dep / ns; }
    a.depth[o] = dep;
    a.seg[o] = segv;
    if (a.u8) {  // (rgb * 255).clamp(0, 255).to(torch.uint8) of the rgb this call's dtype would hold
      unsigned char* out = reinterpret_cast<unsigned char*>(a.rgb);
#pragma unroll
      for (int k = 0; k < 3; k++) {
        REAL x;
        if (a.rgb_f32) x = (REAL)((float)c[k] * 255.0f);
        else x = c[k] * (REAL)255;
        x = x < 0 ? (REAL)0 : (x > (REAL)255 ? (REAL)255 : x);
        out[o * 3 + k] = (unsigned char)(int)x;
      }
    } else if (a.rgb_f32) {
      float* out = reinterpret_cast<float*>(a.rgb);
#pragma unroll
      for (int k = 0; k < 3; k++) out[o * 3 + k] = (float)c[k];
    } else {
      REAL* out = reinterpret_cast<REAL*>(a.rgb);
#pragma unroll
      for (int k = 0; k < 3; k++) out[o * 3 + k] = c[k];
    }
  }
}
