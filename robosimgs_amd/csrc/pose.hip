// pose.hip -- the backward of transform.hip for gfx950 (include/mgs_pose.h): from the cotangents of the posed Gaussians,
// the gradient of every group's pose (in the tangent space: v_omega, v_t, v_lambda) and of the Gaussians at rest.
//   kernel 1  one wave per 64 consecutive Gaussians, the forward kernel's shape: 44 B of posed state and 44 B of cotangent
//             per Gaussian, the 192-byte SH rows (posed and cotangent) of MOVING Gaussians staged through LDS when they
//             hold 16 coefficients (shorter rows are read per lane); every cotangent row only when the rest-pose gradient
//             is asked for.  Each lane forms its seven pose addends; the wave walks the distinct group ids it holds
//             (ballot + readfirstlane), sums each id's lanes with a fixed xor shuffle tree and stores one row
//             (gid, 7 floats) per id with plain vector stores, and the number of rows.
//   kernel 2  one wave per (group, chunk of 64 of those waves): lane l scans wave l's rows for the group's, then a fixed
//             xor tree in fp64; one fp64 partial per (group, chunk).
//   kernel 3  one wave per group: lane l sums chunks l, l + 64, ... in order, the same tree.  Writes v_pose, a zero row
//             for a group nobody belongs to.
// No float atomics: the same bits in every run.  Nothing in the workspace is read that this call did not write.
#include "mgs_common.h"
#include "sh_staging.h"
#include "../../include/mgs_pose.h"

namespace mgs {
namespace {

constexpr int kBlock = 64;            // one wave per workgroup (see transform.hip)
constexpr int kXformFloats = 20;      // M[9] (= s R, row-major), t[3], q_R[4] (wxyz), s, pad[3]
constexpr int kShRotFloats = 84;      // 3x3 + 5x5 + 7x7 (+1 pad), row-major, degree 1..3
constexpr int kPoseFloats = 8;        // v_omega[3], v_t[3], v_lambda, 0

// The generators L_k^(l) = d/d_eps M_l(exp(eps [e_k]x)) at 0 of the real-SH rotation in the renderer's basis order
// (SURVEY.md A.2 step 6).  Antisymmetric: an entry {a, b, v} stands for L[a][b] = v and L[b][a] = -v, with a < b the
// coefficient index above the DC term (degree 1: 0..2, degree 2: 3..7, degree 3: 8..14).  Axis x and y have 1 / 3 / 5
// such pairs at degree 1 / 2 / 3, axis z 1 / 2 / 3.  robosimgs_amd/pose.py: SH_GENERATORS mirrors this table.
constexpr float kSqrt3 = 1.7320508075688772f;        // sqrt(3)
constexpr float kSqrt6 = 2.4494897427831779f;        // sqrt(6)
constexpr float kSqrt3_2 = 1.2247448713915890f;      // sqrt(3/2)
constexpr float kSqrt5_2 = 1.5811388300841898f;      // sqrt(5/2)
struct ShGen { int a, b; float v; };
constexpr int kGenPairs = 9;
__device__ constexpr ShGen kShGen[3][kGenPairs] = {
    {{0, 1, 1.f},                                                              // x, degree 1
     {3, 6, 1.f}, {4, 5, kSqrt3}, {4, 7, 1.f},                                 //    degree 2
     {8, 13, kSqrt3_2}, {9, 12, kSqrt5_2}, {9, 14, kSqrt3_2}, {10, 11, kSqrt6}, {10, 13, kSqrt5_2}},
    {{1, 2, 1.f},                                                              // y
     {3, 4, -1.f}, {5, 6, kSqrt3}, {6, 7, 1.f},
     {8, 9, -kSqrt3_2}, {9, 10, -kSqrt5_2}, {11, 12, kSqrt6}, {12, 13, kSqrt5_2}, {13, 14, kSqrt3_2}},
    {{0, 2, 1.f},                                                              // z (0 entries: padding)
     {3, 7, 2.f}, {4, 6, 1.f}, {0, 0, 0.f},
     {8, 14, 3.f}, {9, 13, 2.f}, {10, 12, 1.f}, {0, 0, 0.f}, {0, 0, 0.f}},
};

template <bool SH, bool STAGED, bool REST>
__global__ __launch_bounds__(kBlock) void pose_bwd_kernel(
    int n, const float* __restrict__ means, const float* __restrict__ quats, const float* __restrict__ scales,
    int sh_degree, int stride_f, const float* __restrict__ sh, const int32_t* __restrict__ group_ids, int n_groups,
    const float* __restrict__ xforms, const float* __restrict__ sh_rot, const float* __restrict__ ct_means,
    const float* __restrict__ ct_quats, const float* __restrict__ ct_scales, const float* __restrict__ ct_sh,
    float* __restrict__ v_means, float* __restrict__ v_quats, float* __restrict__ v_scales, float* __restrict__ v_sh,
    int rows_per_wave, int* __restrict__ counts, float4* __restrict__ rows) {
  __shared__ float4 lds[(SH && STAGED) ? kShWaveSlots : 1];
  const int g0 = blockIdx.x * kBlock;
  const unsigned lane = threadIdx.x;
  const int g = g0 + (int)lane;
  int gid = -1;
  if (g < n) gid = group_ids ? group_ids[g] : 0;
  const bool moving = g < n && gid >= 0 && gid < n_groups;
  const float* X = xforms + (size_t)(moving ? gid : 0) * kXformFloats;
  float acc[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};      // this lane's addends: omega[3], t[3], lambda

  if (g < n) {
    float pb[3] = {0.f, 0.f, 0.f}, sb[3] = {0.f, 0.f, 0.f};
    float4 qb = make_float4(0.f, 0.f, 0.f, 0.f);
    if (ct_means) { pb[0] = ct_means[3 * (size_t)g]; pb[1] = ct_means[3 * (size_t)g + 1]; pb[2] = ct_means[3 * (size_t)g + 2]; }
    if (ct_quats) qb = reinterpret_cast<const float4*>(ct_quats)[g];
    if (ct_scales) { sb[0] = ct_scales[3 * (size_t)g]; sb[1] = ct_scales[3 * (size_t)g + 1]; sb[2] = ct_scales[3 * (size_t)g + 2]; }
    float vp[3] = {pb[0], pb[1], pb[2]}, vs[3] = {sb[0], sb[1], sb[2]};
    float4 vq = qb;
    if (moving) {
      if (ct_means) {
        float d[3];
#pragma unroll
        for (int r = 0; r < 3; ++r) d[r] = means[3 * (size_t)g + r] - X[9 + r];      // p' - t
        acc[0] = d[1] * pb[2] - d[2] * pb[1];
        acc[1] = d[2] * pb[0] - d[0] * pb[2];
        acc[2] = d[0] * pb[1] - d[1] * pb[0];
        acc[3] = pb[0]; acc[4] = pb[1]; acc[5] = pb[2];
        acc[6] = pb[0] * d[0] + pb[1] * d[1] + pb[2] * d[2];
      }
      if (ct_quats) {
        const float4 q = reinterpret_cast<const float4*>(quats)[g];     // q' = (w, x, y, z) in (x, y, z, w)
        // <ct_q, e_k (x) q'>:  e_x (x) q' = (-x, w, -z, y),  e_y (x) q' = (-y, z, w, -x),  e_z (x) q' = (-z, -y, x, w)
        acc[0] += 0.5f * (qb.y * q.x - qb.x * q.y + qb.w * q.z - qb.z * q.w);
        acc[1] += 0.5f * (qb.z * q.x - qb.x * q.z + qb.y * q.w - qb.w * q.y);
        acc[2] += 0.5f * (qb.w * q.x - qb.x * q.w + qb.z * q.y - qb.y * q.z);
      }
      if (ct_scales) {
        float dot = 0.f;
#pragma unroll
        for (int r = 0; r < 3; ++r) dot += sb[r] * scales[3 * (size_t)g + r];
        acc[6] += dot;
      }
      if constexpr (REST) {
#pragma unroll
        for (int c = 0; c < 3; ++c) vp[c] = X[c] * pb[0] + X[3 + c] * pb[1] + X[6 + c] * pb[2];       // (s R)^T ct_p
        const float aw = X[12], ax = -X[13], ay = -X[14], az = -X[15], s = X[16];                       // conj(q_R)
        vq = make_float4(aw * qb.x - ax * qb.y - ay * qb.z - az * qb.w, aw * qb.y + ax * qb.x + ay * qb.w - az * qb.z,
                         aw * qb.z - ax * qb.w + ay * qb.x + az * qb.y, aw * qb.w + ax * qb.z - ay * qb.y + az * qb.x);
#pragma unroll
        for (int r = 0; r < 3; ++r) vs[r] = s * sb[r];
      }
    }
    if constexpr (REST) {
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        v_means[3 * (size_t)g + r] = vp[r];
        v_scales[3 * (size_t)g + r] = vs[r];
      }
      reinterpret_cast<float4*>(v_quats)[g] = vq;
    }
  }

  if constexpr (SH) {
    const int rows_here = min(kBlock, n - g0);
    if (!ct_sh) {
      if constexpr (REST) {                                   // a null cotangent is zero: so is its gradient
        float* dst = v_sh + (size_t)g0 * stride_f;
        for (int i = lane; i < rows_here * stride_f; i += kBlock) dst[i] = 0.f;
      }
    } else {
      const unsigned long long mask_mov = ballot(moving);
      const unsigned long long need_ct = REST ? ballot(g < n) : mask_mov;
      if (need_ct != 0ull) {
        const int kc = (sh_degree + 1) * (sh_degree + 1) - 1;       // coefficients above the DC term
        float cp[45], cb[45];                                        // posed row, cotangent row: 15 x rgb
        float* row;                                                  // this lane's cotangent row
        if constexpr (STAGED) {
          row = reinterpret_cast<float*>(lds + lane * kShPitchF4);
          if (mask_mov != 0ull) {
            sh_rows_to_lds(sh, g0, n, mask_mov, lds);
            __syncthreads();
#pragma unroll
            for (int i = 0; i < 45; ++i) cp[i] = (moving && i < kc * 3) ? row[3 + i] : 0.f;
            __syncthreads();
          } else {
#pragma unroll
            for (int i = 0; i < 45; ++i) cp[i] = 0.f;
          }
          sh_rows_to_lds(ct_sh, g0, n, need_ct, lds);
          __syncthreads();
        } else {
          const float* prow = sh + (size_t)(moving ? g : 0) * stride_f;
#pragma unroll
          for (int i = 0; i < 45; ++i) cp[i] = (moving && i < kc * 3) ? prow[3 + i] : 0.f;
          row = const_cast<float*>(ct_sh) + (size_t)(g < n ? g : 0) * stride_f;
        }
        const bool have = REST ? g < n : moving;
#pragma unroll
        for (int i = 0; i < 45; ++i) cb[i] = (have && i < kc * 3) ? row[3 + i] : 0.f;
        float o[45];
#pragma unroll
        for (int i = 0; i < 45; ++i) o[i] = cb[i];
        if (moving && sh_degree >= 1) {
          // sum_ch <ct_c, L_k c'> = sum over the pairs of v (ct_a c'_b - ct_b c'_a); rows above the degree are zero
#pragma unroll
          for (int k = 0; k < 3; ++k) {
            float w = acc[k];
#pragma unroll
            for (int e = 0; e < kGenPairs; ++e) {
              const int a = 3 * kShGen[k][e].a, b = 3 * kShGen[k][e].b;
              const float v = kShGen[k][e].v;
              if (v != 0.f) {
                float sp = 0.f;
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) sp += cb[a + ch] * cp[b + ch] - cb[b + ch] * cp[a + ch];
                w += v * sp;
              }
            }
            acc[k] = w;
          }
          if constexpr (REST) {
            const float* M = sh_rot + (size_t)gid * kShRotFloats;
            // M_l^T ct_c,l: degree 1 coefficients 1..3 (cb[0..8]), degree 2: 4..8 (cb[9..23]), degree 3: 9..15 (cb[24..44])
#pragma unroll
            for (int j = 0; j < 3; ++j)
#pragma unroll
              for (int ch = 0; ch < 3; ++ch) {       // (from +0, as below: a zero cotangent gives +0 whatever M's signs)
                float t = 0.f;
#pragma unroll
                for (int k = 0; k < 3; ++k) t = fmaf(M[3 * k + j], cb[3 * k + ch], t);
                o[3 * j + ch] = t;
              }
            if (sh_degree >= 2) {
#pragma unroll
              for (int j = 0; j < 5; ++j)
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) {
                  float t = 0.f;
#pragma unroll
                  for (int k = 0; k < 5; ++k) t = fmaf(M[9 + 5 * k + j], cb[9 + 3 * k + ch], t);
                  o[9 + 3 * j + ch] = t;
                }
            }
            if (sh_degree >= 3) {
#pragma unroll
              for (int j = 0; j < 7; ++j)
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) {
                  float t = 0.f;
#pragma unroll
                  for (int k = 0; k < 7; ++k) t = fmaf(M[34 + 7 * k + j], cb[24 + 3 * k + ch], t);
                  o[24 + 3 * j + ch] = t;
                }
            }
          }
        }
        if constexpr (REST) {
          if constexpr (STAGED) {
            if (moving) {
#pragma unroll
              for (int i = 0; i < 45; ++i)
                if (i < kc * 3) row[3 + i] = o[i];
            }
            __syncthreads();
            sh_rows_from_lds<false>(v_sh, g0, n, lds);             // every row of the wave: need_ct was all of them
          } else if (g < n) {
            float* dst = v_sh + (size_t)g * stride_f;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) dst[ch] = row[ch];          // DC term
#pragma unroll
            for (int i = 0; i < 45; ++i)
              if (i < kc * 3) dst[3 + i] = o[i];
            for (int i = 3 + kc * 3; i < stride_f; ++i) dst[i] = row[i];   // coefficients above the active degree
          }
        }
      }
    }
  }

  // per group id present in the wave: a fixed xor tree over its lanes, one row (gid, 7 floats) from lane 0
  unsigned long long rem = ballot(moving);
  int slot = 0;
  float4* out = rows + (size_t)blockIdx.x * rows_per_wave * 2;
  while (rem != 0ull) {
    const int leader = __builtin_amdgcn_readfirstlane(__ffsll((long long)rem) - 1);
    const int cur = __builtin_amdgcn_readlane(gid, leader);
    const bool mine = moving && gid == cur;
    rem &= ~ballot(mine);
    float r[7];
#pragma unroll
    for (int k = 0; k < 7; ++k) {
      float v = mine ? acc[k] : 0.f;
#pragma unroll
      for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
      r[k] = v;
    }
    if (lane == 0 && slot < rows_per_wave) {
      out[2 * slot] = make_float4(__int_as_float(cur), r[0], r[1], r[2]);
      out[2 * slot + 1] = make_float4(r[3], r[4], r[5], r[6]);
    }
    ++slot;
  }
  if (lane == 0) counts[blockIdx.x] = min(slot, rows_per_wave);
}

// Stage 2: one wave per (group, chunk of 64 waves of stage 1).  Lane l scans the rows of wave 64 chunk + l for the group's
// (a wave holds at most one row per group), then a fixed xor tree in fp64.
__global__ __launch_bounds__(kBlock) void pose_chunk_kernel(int waves, int rows_per_wave, int chunks,
                                                            const int* __restrict__ counts,
                                                            const float4* __restrict__ rows, double* __restrict__ partial) {
  const int grp = blockIdx.x, lane = threadIdx.x;
  for (int ch = blockIdx.y; ch < chunks; ch += gridDim.y) {
    const int w = ch * kBlock + lane;
    double s[7] = {0., 0., 0., 0., 0., 0., 0.};
    if (w < waves) {
      const int c = min(counts[w], rows_per_wave);
      const float4* in = rows + (size_t)w * rows_per_wave * 2;
      for (int j = 0; j < c; ++j) {
        const float4 a = in[2 * j];
        if (__float_as_int(a.x) == grp) {
          const float4 b = in[2 * j + 1];
          s[0] = (double)a.y; s[1] = (double)a.z; s[2] = (double)a.w;
          s[3] = (double)b.x; s[4] = (double)b.y; s[5] = (double)b.z; s[6] = (double)b.w;
          break;
        }
      }
    }
#pragma unroll
    for (int k = 0; k < 7; ++k) {
#pragma unroll
      for (int d = 32; d >= 1; d >>= 1) s[k] += __shfl_xor(s[k], d);
    }
    if (lane == 0) {
      double* out = partial + ((size_t)grp * chunks + ch) * kPoseFloats;
#pragma unroll
      for (int k = 0; k < 7; ++k) out[k] = s[k];
      out[7] = 0.;
    }
  }
}

// Stage 3: one wave per group sums the chunks' fp64 partials: lane l takes chunks l, l + 64, ... in order, then the same
// tree.  Writes the group's row of v_pose (zeros where nobody belongs to the group, or there is no Gaussian at all).
__global__ __launch_bounds__(kBlock) void pose_final_kernel(int chunks, const double* __restrict__ partial,
                                                            float* __restrict__ v_pose) {
  const int grp = blockIdx.x, lane = threadIdx.x;
  double s[7] = {0., 0., 0., 0., 0., 0., 0.};
  for (int ch = lane; ch < chunks; ch += kBlock) {
    const double* in = partial + ((size_t)grp * chunks + ch) * kPoseFloats;
#pragma unroll
    for (int k = 0; k < 7; ++k) s[k] += in[k];
  }
#pragma unroll
  for (int k = 0; k < 7; ++k) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) s[k] += __shfl_xor(s[k], d);
  }
  if (lane == 0) {
    float* out = v_pose + (size_t)grp * kPoseFloats;
#pragma unroll
    for (int k = 0; k < 7; ++k) out[k] = (float)s[k];
    out[7] = 0.f;
  }
}

struct PoseLayout { size_t counts, rows, partial, total; int waves, rows_per_wave, chunks; };

PoseLayout pose_layout(int n, int n_groups) {
  PoseLayout L;
  L.waves = (int)(((long long)n + kBlock - 1) / kBlock);
  L.rows_per_wave = n_groups < kBlock ? n_groups : kBlock;
  L.chunks = (L.waves + kBlock - 1) / kBlock;
  Bump b(1);
  L.counts = b.take((size_t)L.waves * sizeof(int));
  L.rows = b.take((size_t)L.waves * L.rows_per_wave * 2 * sizeof(float4));
  L.partial = b.take((size_t)L.chunks * n_groups * kPoseFloats * sizeof(double));
  L.total = b.total;
  return L;
}

}  // namespace
}  // namespace mgs

using namespace mgs;

extern "C" size_t mgs_pose_bwd_workspace_bytes(int n, int n_groups) {
  if (n < 0 || n_groups < 1) return 0;
  return pose_layout(n, n_groups).total;
}

extern "C" int mgs_pose_bwd(int n, const float* means, const float* quats, const float* scales, int sh_degree,
                            int coeff_stride, const float* sh_coeffs, const int32_t* group_ids, int n_groups,
                            const float* xforms, const float* sh_rot, const float* ct_means, const float* ct_quats,
                            const float* ct_scales, const float* ct_sh, float* v_means, float* v_quats, float* v_scales,
                            float* v_sh, float* v_pose, void* workspace, size_t workspace_bytes, mgs_stream_t stream) {
  MGS_REQUIRE(n >= 0, "pose_bwd: n is negative (%d)", n);
  MGS_REQUIRE(n_groups >= 1, "pose_bwd: n_groups %d, at least one group is needed", n_groups);
  MGS_REQUIRE(means && quats && scales, "pose_bwd: a posed array (means, quats, scales) is null");
  MGS_REQUIRE(xforms, "pose_bwd: xforms is null");
  MGS_REQUIRE(v_pose, "pose_bwd: v_pose is null");
  MGS_REQUIRE(!sh_coeffs || (sh_degree >= 0 && sh_degree <= 3), "pose_bwd: sh_degree %d is outside 0..3", sh_degree);
  MGS_REQUIRE(!sh_coeffs || coeff_stride >= (sh_degree + 1) * (sh_degree + 1),
              "pose_bwd: coeff_stride %d is too short for the %d coefficients of degree %d", coeff_stride,
              (sh_degree + 1) * (sh_degree + 1), sh_degree);
  MGS_REQUIRE(!sh_coeffs || sh_degree == 0 || sh_rot, "pose_bwd: degree >= 1 needs sh_rot");
  MGS_REQUIRE(sh_coeffs || (!ct_sh && !v_sh), "pose_bwd: an SH cotangent or gradient without posed SH rows");
  const bool rest = v_means || v_quats || v_scales || v_sh;
  MGS_REQUIRE(!rest || (v_means && v_quats && v_scales && (v_sh != nullptr) == (sh_coeffs != nullptr)),
              "pose_bwd: rest-pose gradients given only in part (v_means, v_quats, v_scales, and v_sh with SH rows)");
  MGS_REQUIRE(workspace, "pose_bwd: workspace is null");
  const PoseLayout L = pose_layout(n, n_groups);
  MGS_REQUIRE(workspace_bytes >= L.total, "pose_bwd: workspace of %zu bytes, %zu needed", workspace_bytes, L.total);
  hipStream_t s = (hipStream_t)stream;
  char* ws = static_cast<char*>(workspace);
  int* counts = reinterpret_cast<int*>(ws + L.counts);
  float4* rows = reinterpret_cast<float4*>(ws + L.rows);
  const int stride_f = coeff_stride * 3;
  if (L.waves > 0) {
    with_bool(sh_coeffs != nullptr, [&](auto sh) {
      with_bool(sh_coeffs && coeff_stride == 16, [&](auto staged) {
        with_bool(rest, [&](auto rest_c) {
          constexpr bool SH = decltype(sh)::value;
          if constexpr (SH || !decltype(staged)::value)       // (no SH rows: nothing to stage)
            hipLaunchKernelGGL((pose_bwd_kernel<SH, decltype(staged)::value, decltype(rest_c)::value>), dim3(L.waves),
                               dim3(kBlock), 0, s, n, means, quats, scales, SH ? sh_degree : 0, SH ? stride_f : 0,
                               sh_coeffs, group_ids, n_groups, xforms, SH ? sh_rot : nullptr, ct_means, ct_quats,
                               ct_scales, ct_sh, v_means, v_quats, v_scales, v_sh, L.rows_per_wave, counts, rows);
        });
      });
    });
    int rc = check_launch("pose_bwd");
    if (rc) return rc;
  }
  double* partial = reinterpret_cast<double*>(ws + L.partial);
  if (L.chunks > 0) {
    hipLaunchKernelGGL(pose_chunk_kernel, dim3(n_groups, L.chunks < 1024 ? L.chunks : 1024), dim3(kBlock), 0, s, L.waves,
                       L.rows_per_wave, L.chunks, counts, rows, partial);
    int rc = check_launch("pose_bwd");
    if (rc) return rc;
  }
  hipLaunchKernelGGL(pose_final_kernel, dim3(n_groups), dim3(kBlock), 0, s, L.chunks, partial, v_pose);
  return check_launch("pose_bwd");
}
