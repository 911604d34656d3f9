// khr_fuse_math.h — the arithmetic of the projective update of ONE voxel (hydra::ProjectiveIntegrator::updateVoxel and what
// it calls), stated once.  k_fuse, k_fuse2 and k_fuse_obj (khr_kernels_fuse.h) are three schedules of this arithmetic: each
// decides what it keeps in registers, when it gathers and what it stores where, and takes every value and every decision of
// the update from here.  The helpers take values and give values: no map or image memory is touched in this file.
//
// Every DECISION (in front of the camera, in range, in the image, interpolation mode, sdf >= -truncation, inside the band,
// dynamic-mask pixel, weight > 0) is evaluated with the reference's operations in the reference's order; the divisions
// behind them share one refined reciprocal of the voxel depth and use the correctly rounded rcp-Newton-FMA sequence.
// EXACT = false relaxes only VALUES (measurement weight, running average); EXACT = true keeps them bit-identical to the
// CPU oracle.  A correction to one of these belongs here and reaches every kernel.
#pragma once
#include "khr_device.h"

namespace khr {

__device__ inline void interpPixels(float u, float v, int W, int H, int* px, float* du, float* dv) {
  const int u0 = static_cast<int>(floorf(u)), v0 = static_cast<int>(floorf(v));
  const int u1 = min(u0 + 1, W - 1), v1 = min(v0 + 1, H - 1);
  *du = u - static_cast<float>(u0);
  *dv = v - static_cast<float>(v0);
  px[0] = v0 * W + u0;
  px[1] = v1 * W + u0;
  px[2] = v0 * W + u1;
  px[3] = v1 * W + u1;
}

__device__ inline int interpWeights(float du, float dv, bool use_nearest, float* w4) {
  int best;
  if (use_nearest) {
    const int nearest = (du >= 0.5f ? 2 : 0) + (dv >= 0.5f ? 1 : 0);
#pragma unroll
    for (int k = 0; k < 4; ++k) w4[k] = (k == nearest) ? 1.f : 0.f;
    best = nearest;
  } else {
    w4[0] = (1.f - du) * (1.f - dv);
    w4[1] = (1.f - du) * dv;
    w4[2] = du * (1.f - dv);
    w4[3] = du * dv;
    best = 0;
#pragma unroll
    for (int k = 1; k < 4; ++k)
      if (w4[k] > w4[best]) best = k;
  }
  return best;
}

// y ~ 1 / b: v_rcp_f32 (1 ulp) + one Newton step.  For normal b this is the reciprocal hipcc's IEEE division uses.
__device__ inline float rcpRefined(float b) {
  const float y = __builtin_amdgcn_rcpf(b);
  const float e = __builtin_fmaf(-b, y, 1.f);
  return __builtin_fmaf(e, y, y);
}
// correctly rounded a / b from y = rcpRefined(b): the quotient / residual steps of hipcc's expansion of an IEEE f32
// division (v_div_scale / v_div_fmas / v_div_fixup only matter for operands near the ends of the exponent range)
__device__ inline float divExact(float a, float b, float y) {
  float q = a * y;
  float r = __builtin_fmaf(-b, q, a);
  q = __builtin_fmaf(r, y, q);
  r = __builtin_fmaf(-b, q, a);
  return __builtin_fmaf(r, y, q);
}

// ---- voxel projection: camera-frame position, range validity, pixel ------------------------------------------------
struct VoxelProj {
  bool ok;       // in front of the camera, inside [min_range, max_range], inside the image
  float range;   // the voxel's range: its depth (range_mode 0) or the length of its ray
  float yz;      // rcpRefined(depth)
  float uc, vc;  // the projected pixel; (0, 0) for a voxel that is not ok: such a lane gathers pixel (0, 0)
};
// pxy: the x-y part of the camera-frame position (R[3c] x + R[3c + 1] y), the z step adds R[3c + 2] pz and t[c] in that order
// (the operation order of the reference restatement, so the projected pixel is bit-identical).  CAM: a FuseFrame.
template <class CAM>
__device__ __forceinline__ VoxelProj projectVoxel(const CAM& f, const float (&pxy)[3], float pz, float Wm1, float Hm1, int range_mode) {
  float pc[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) pc[c] = (pxy[c] + f.R[3 * c + 2] * pz) + f.t[c];
  VoxelProj p;
  bool ok = pc[2] > 0.f;
  p.range = range_mode == 0 ? pc[2] : sqrtf((pc[0] * pc[0] + pc[1] * pc[1]) + pc[2] * pc[2]);
  ok = ok && !(p.range < f.min_range || p.range > f.max_range);
  p.yz = rcpRefined(pc[2]);
  const float u = divExact(pc[0] * f.fx, pc[2], p.yz) + f.cx;
  const float v = divExact(pc[1] * f.fy, pc[2], p.yz) + f.cy;
  // ceil(u) >= W || floor(u) < 0  <=>  u > W - 1 || u < 0  (W - 1 is an integer-valued float); x - y >= 0 <=> x >= y
  // holds exactly in IEEE arithmetic, so the four tests are one min3 / min / compare.
  // (`&`, and `&&` above: the same value either way, but k_fuse sits on its register budget and is sensitive to the form --
  // `&&` here costs its flagship instantiation 8 VALU and 10 wait instructions, `&` above puts the instantiation for
  // non-default switches into scratch memory; profiles/update_arithmetic.txt)
  ok = ok & (fminf(fminf(u, v), fminf(Wm1 - u, Hm1 - v)) >= 0.f);
  p.ok = ok;
  p.uc = ok ? u : 0.f;
  p.vc = ok ? v : 0.f;
  return p;
}

// ---- byte offsets of the two range-gather pixel pairs (u0, v0)-(u0 + 1, v0) and (u0, v1)-(u0 + 1, v1) -------------------
// 0 <= uc <= W - 1 and 0 <= vc <= H - 1 (projectVoxel), so floor == truncation.  W4 = 4 W, the row pitch in bytes.
// MUL24: 24-bit multiplies (rows and row pitch are far below 2^24): the full 32-bit multiply-add only exists as
// v_mad_u64_u32, whose 64-bit addend drags an unrelated register into the instruction -- when that register is the target of
// a load in flight, the compiler has to wait for it (seen in the ISA of k_fuse's phase 1: vmcnt(2))
struct PairOffsets {
  uint32_t o0, o1;
};
template <bool MUL24>
__device__ __forceinline__ PairOffsets pairOffsets(float uc, float vc, int H, uint32_t W4) {
  const uint32_t u0 = static_cast<uint32_t>(static_cast<int>(uc)), v0 = static_cast<uint32_t>(static_cast<int>(vc));
  const uint32_t v1 = min(v0 + 1u, static_cast<uint32_t>(H - 1));
  PairOffsets o;
  o.o0 = (MUL24 ? __umul24(v0, W4) : v0 * W4) + u0 * 4u;
  o.o1 = (MUL24 ? __umul24(v1, W4) : v1 * W4) + u0 * 4u;
  return o;
}

// ---- surface sample: interpolated range at the voxel's pixel, signed distance, band decisions ---------------------------
struct SurfaceSample {
  float r0, r1, r2, r3;  // pixel order of the reference: (u0,v0) (u0,v1) (u1,v0) (u1,v1) with u1 = min(u0 + 1, W - 1)
  float w0, w1, w2, w3;  // their bilinear weights
  bool last_col, use_nearest, hi_u, hi_v;
  float dist_surface, sdf;
  bool ok, in_band;  // the voxel is updated; ... and lies inside the truncation band
};
// (a0, a1) = the pixel pair (u0, v0)-(u0 + 1, v0), (b0, b1) = (u0, v1)-(u0 + 1, v1); ok = projectVoxel's;
// interp: 0 nearest, 1 bilinear, 2 adaptive (nearest where the four samples differ by more than adaptive_diff)
__device__ __forceinline__ SurfaceSample sampleSurface(bool ok, float a0, float a1, float b0, float b1, float uc, float vc, int W, int interp,
                                                       float adaptive_diff, float voxel_range, float min_range, float max_range, float trunc) {
  SurfaceSample s;
  const float du = __builtin_amdgcn_fractf(uc), dv = __builtin_amdgcn_fractf(vc);  // x - floor(x), exact for x >= 0
  s.last_col = static_cast<uint32_t>(static_cast<int>(uc)) >= static_cast<uint32_t>(W - 1);
  s.r0 = a0;
  s.r1 = b0;
  s.r2 = s.last_col ? a0 : a1;
  s.r3 = s.last_col ? b0 : b1;
  s.use_nearest = interp == 0;
  if (interp == 2) {
    const float mn = fminf(fminf(s.r0, s.r1), fminf(s.r2, s.r3));
    const float mx = fmaxf(fmaxf(s.r0, s.r1), fmaxf(s.r2, s.r3));
    s.use_nearest = s.use_nearest || (mx - mn > adaptive_diff);
  }
  s.hi_u = du >= 0.5f;
  s.hi_v = dv >= 0.5f;
  const float r_near = s.hi_u ? (s.hi_v ? s.r3 : s.r2) : (s.hi_v ? s.r1 : s.r0);
  const float omu = 1.f - du, omv = 1.f - dv;
  s.w0 = omu * omv;
  s.w1 = omu * dv;
  s.w2 = du * omv;
  s.w3 = du * dv;
  const float r_bil = ((s.w0 * s.r0 + s.w1 * s.r1) + s.w2 * s.r2) + s.w3 * s.r3;
  s.dist_surface = s.use_nearest ? r_near : r_bil;
  ok = ok & (s.dist_surface >= min_range) & !(s.dist_surface > max_range);
  s.sdf = s.dist_surface - voxel_range;
  s.ok = ok & !(s.sdf < -trunc);
  s.in_band = s.ok & (fabsf(s.sdf) < trunc);
  return s;
}

// byte offset of the dynamic-mask pixel, interpolateID(mask): the pixel of the largest weight (first maximum), or the nearest
__device__ __forceinline__ uint32_t maskPixelOffset(const SurfaceSample& s, uint32_t o0, uint32_t o1) {
  int best;
  if (s.use_nearest) {
    best = (s.hi_u ? 2 : 0) + (s.hi_v ? 1 : 0);
  } else {
    best = 0;
    float bw = s.w0;
    if (s.w1 > bw) { bw = s.w1; best = 1; }
    if (s.w2 > bw) { bw = s.w2; best = 2; }
    if (s.w3 > bw) { bw = s.w3; best = 3; }
  }
  const uint32_t uo = ((best & 2) && !s.last_col) ? 4u : 0u;
  return ((best & 1) ? o1 : o0) + uo;
}

// measurement weight (computeWeight): fx fy vs^2 / z^4, linear drop-off behind the surface.  yz = rcpRefined(depth),
// den = trunc - dropoff_eps, yden = rcpRefined(den).  w > 0 is the same decision in both modes: the factors are positive
// normal numbers far from underflow, so the product is zero exactly when trunc + sdf == 0
template <bool EXACT>
__device__ __forceinline__ float measurementWeight(float vs, float fxfy, float depth, float yz, float sdf, float trunc, float dropoff_eps, float den,
                                                   float yden, bool use_dropoff, bool const_weight) {
  float w;
  if (EXACT) {
    const float qd = divExact(vs, depth, yz);
    w = fxfy * (qd * qd);
    if (!const_weight) {
      const float z2 = depth * depth;
      w = divExact(w, z2, rcpRefined(z2));
    }
    if (use_dropoff && sdf < -dropoff_eps) w = fmaxf(w * divExact(trunc + sdf, den, yden), 0.f);
  } else {
    const float qd = vs * yz;
    w = fxfy * (qd * qd);
    if (!const_weight) w = w * (yz * yz);
    if (use_dropoff && sdf < -dropoff_eps) w = fmaxf(w * ((trunc + sdf) * yden), 0.f);
  }
  return w;
}

// the voxel's distance and weight after a measurement of weight w at signed distance sdf
struct VoxelAverage {
  float d_new, w_new;
};
template <bool EXACT>
__device__ __forceinline__ VoxelAverage runningAverage(float d_old, float w_old, float sdf, float w, float trunc, float max_weight) {
  const float sdf_c = fmaxf(fminf(trunc, sdf), -trunc);
  const float tot = w_old + w;
  VoxelAverage r;
  if (EXACT) {
    r.d_new = divExact(d_old * w_old + sdf_c * w, tot, rcpRefined(tot));
  } else {
    r.d_new = __builtin_fmaf(d_old, w_old, sdf_c * w) * __builtin_amdgcn_rcpf(tot);
  }
  r.w_new = fminf(tot, max_weight);
  return r;
}

// colour of an in-band voxel: the image colours c4 (pixel order of interpPixels) interpolated with w4, rounded to 8 bits, and
// averaged into the voxel's colour co.  wv = the voxel's blend weight (before or after the update: khr_config.color_blend_weight),
// w = the measurement weight.
__device__ __forceinline__ uint32_t blendColor(const uint32_t (&c4)[4], const float (&w4)[4], uint32_t co, float wv, float w) {
  float acc[3] = {0.f, 0.f, 0.f};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const uint32_t c = c4[k];
    acc[0] = acc[0] + w4[k] * static_cast<float>(c & 0xffu);
    acc[1] = acc[1] + w4[k] * static_cast<float>((c >> 8) & 0xffu);
    acc[2] = acc[2] + w4[k] * static_cast<float>((c >> 16) & 0xffu);
  }
  const float tot = wv + w;
  const float ytot = rcpRefined(tot);
  uint32_t out = 0xff000000u;
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    const float cn = static_cast<float>(toU8(acc[ch]));
    const float cv = static_cast<float>((co >> (8 * ch)) & 0xffu);
    out |= static_cast<uint32_t>(toU8(divExact(cv * wv + cn * w, tot, ytot))) << (8 * ch);
  }
  return out;
}

}  // namespace khr
