// micro-benchmark: what do the SCALAR instructions of the forward raster's hand-written blend body cost?
//
// raster_fwd_kernel walks a wave-private LDS queue: per queued Gaussian `at = s_ff1(rest)`, `s_bitset0`, three broadcast
// ds_read_b128, then up to four quadrant bodies (raster_fwd.hip: blend_pixel_safe_asm, 15 vector instructions per 64
// pairs), each behind `s_bitcmp1_b64 reach[k], at` and a branch.  This program prices that walk -- "form L" of
// queue_feed.hip, brought up to the lane-mask walk -- with the body in four forms that compute the same bits:
//   form 0  the body as it shipped before this benchmark was written: seven scalar issue slots besides the test and
//           the branch (s_mov exec, alive | s_nop 0 | s_xor vcc, vcc, acc | s_andn2 alive | s_cselect vcc | s_and quad |
//           s_mov exec, -1) and an SGPR pair for `acc`
//   form A  five slots: the polynomial and v_exp run under the full EXEC the body starts with and `s_mov exec, alive`
//           takes the place of the s_nop (the wait state after the transcendental); the closing lanes are
//           vcc & ~exec (the second v_cmpx names EXEC as its scalar destination: no `acc` pair); and
//           `s_cselect_b64 quad, quad, 0` on the SCC of the s_andn2 empties `quad` in one instruction
//   form B  the four bodies of an entry as ONE asm block whose EXEC is restored once, at its end; each body keeps
//           `s_mov exec, alive` at its head and the s_nop, and has form A's other two changes (five slots per body and
//           one per entry: 5.5 per body at 2.08 bodies per entry)
//   form C  four form-A bodies as one asm block (each restores EXEC itself)
// Forms B and C also pay the compiler's `s_nop 0` between two asm statements that share a register once per entry
// instead of four times.  Form B priced lowest at every occupancy and is what raster_fwd.hip ships
// (profiles/raster_scalar/README.md).
// at 4, 5, 6 and 8 waves per SIMD (occupancy forced with dynamic LDS), on synthetic batches shaped like configs[1]:
// 54 queued entries per batch of 64, 2.25 quadrants reached per entry on average, alpha >= 1/255 for ~40 % of the lanes.
// The forms take turns inside the process in an order that rotates from round to round (a fixed order prices the form
// in second place higher, profiles/raster_shared/README.md); the first round is dropped.  Every form's pixels are
// compared with form 0's, bit for bit.
// Reported per form and occupancy: median and minimum over the rounds of the launch time, ns per body per wave and
// SIMD-cycles per vector instruction of the body (15 per body in every form).
//
//   hipcc --offload-arch=gfx950 -O3 -o blend_body_scalar.bin blend_body_scalar.hip && ./blend_body_scalar.bin
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e_)); exit(1); } } while (0)

typedef float f4 __attribute__((ext_vector_type(4)));

struct Px { float T, c0, c1, c2, c3; };
struct Poly { float x, y, xx, xy, yy; };

// ---- form 0 ------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void body_0(Px& p, unsigned long long& alive, unsigned long long& quad, int at, const Poly& pp,
                                       float q0, float q1, float q2, float A, float B, float C, float f0, float f1, float f2,
                                       float f3) {
  float dx, t0, t1;
  unsigned long long acc;
  const float amin = 1.0f / 255.0f, tstop = 1e-4f;
  asm volatile(
      "s_bitcmp1_b64 %[quad], %[at]\n"
      "s_cbranch_scc0 .Lnext0_%=\n"
      "s_mov_b64 exec, %[alive]\n"
      "v_fma_f32 %[t1], %[q1], %[x], %[q0]\n"
      "v_fmac_f32 %[t1], %[q2], %[y]\n"
      "v_fmac_f32 %[t1], %[A], %[xx]\n"
      "v_fmac_f32 %[t1], %[B], %[xy]\n"
      "v_fmac_f32 %[t1], %[C], %[yy]\n"
      "v_exp_f32 %[t1], %[t1]\n"
      "s_nop 0\n"
      "v_cmpx_le_f32 vcc, %[amin], %[t1]\n"
      "v_fma_f32 %[t0], -%[t1], %[T], %[T]\n"
      "v_mul_f32 %[dx], %[t1], %[T]\n"
      "v_cmpx_lt_f32_e64 %[acc], %[tstop], %[t0]\n"
      "v_mov_b32 %[T], %[t0]\n"
      "v_fmac_f32 %[c0], %[dx], %[f0]\n"
      "v_fmac_f32 %[c1], %[dx], %[f1]\n"
      "v_fmac_f32 %[c2], %[dx], %[f2]\n"
      "v_fmac_f32 %[c3], %[dx], %[f3]\n"
      "s_xor_b64 vcc, vcc, %[acc]\n"
      "s_andn2_b64 %[alive], %[alive], vcc\n"
      "s_cselect_b64 vcc, -1, 0\n"
      "s_and_b64 %[quad], %[quad], vcc\n"
      "s_mov_b64 exec, -1\n"
      ".Lnext0_%=:\n"
      : [dx] "=&v"(dx), [t0] "=&v"(t0), [t1] "=&v"(t1), [acc] "=&s"(acc), [alive] "+s"(alive), [quad] "+s"(quad),
        [T] "+v"(p.T), [c0] "+v"(p.c0), [c1] "+v"(p.c1), [c2] "+v"(p.c2), [c3] "+v"(p.c3)
      : [q0] "v"(q0), [q1] "v"(q1), [q2] "v"(q2), [x] "v"(pp.x), [y] "v"(pp.y), [xx] "v"(pp.xx), [xy] "v"(pp.xy), [yy] "v"(pp.yy),
        [A] "v"(A), [B] "v"(B), [C] "v"(C), [f0] "v"(f0), [f1] "v"(f1), [f2] "v"(f2), [f3] "v"(f3), [amin] "s"(amin),
        [tstop] "s"(tstop), [at] "s"(at)
      : "vcc", "scc");
}

// ---- form A: five scalar slots, no `acc` pair ----------------------------------------------------------------------
// EXEC is -1 when the body starts (every body ends with s_mov exec, -1; the walk around it runs with full EXEC), so t1 is
// computed for every lane: closed lanes get a t1, possibly inf, that nothing reads.  From the first v_cmpx on, EXEC is
// what it is in form 0.
__device__ __forceinline__ void body_a(Px& p, unsigned long long& alive, unsigned long long& quad, int at, const Poly& pp,
                                       float q0, float q1, float q2, float A, float B, float C, float f0, float f1, float f2,
                                       float f3) {
  float dx, t0, t1;
  const float amin = 1.0f / 255.0f, tstop = 1e-4f;
  asm volatile(
      "s_bitcmp1_b64 %[quad], %[at]\n"
      "s_cbranch_scc0 .Lnexta_%=\n"
      "v_fma_f32 %[t1], %[q1], %[x], %[q0]\n"
      "v_fmac_f32 %[t1], %[q2], %[y]\n"
      "v_fmac_f32 %[t1], %[A], %[xx]\n"
      "v_fmac_f32 %[t1], %[B], %[xy]\n"
      "v_fmac_f32 %[t1], %[C], %[yy]\n"
      "v_exp_f32 %[t1], %[t1]\n"
      "s_mov_b64 exec, %[alive]\n"                     // the wait state between the transcendental and its reader
      "v_cmpx_le_f32 vcc, %[amin], %[t1]\n"
      "v_fma_f32 %[t0], -%[t1], %[T], %[T]\n"
      "v_mul_f32 %[dx], %[t1], %[T]\n"
      "v_cmpx_lt_f32_e64 exec, %[tstop], %[t0]\n"      // (gfx9: a VOP3 v_cmpx writes its scalar destination AND EXEC)
      "v_mov_b32 %[T], %[t0]\n"
      "v_fmac_f32 %[c0], %[dx], %[f0]\n"
      "v_fmac_f32 %[c1], %[dx], %[f1]\n"
      "v_fmac_f32 %[c2], %[dx], %[f2]\n"
      "v_fmac_f32 %[c3], %[dx], %[f3]\n"
      "s_andn2_b64 vcc, vcc, exec\n"
      "s_andn2_b64 %[alive], %[alive], vcc\n"
      "s_cselect_b64 %[quad], %[quad], 0\n"
      "s_mov_b64 exec, -1\n"
      ".Lnexta_%=:\n"
      : [dx] "=&v"(dx), [t0] "=&v"(t0), [t1] "=&v"(t1), [alive] "+s"(alive), [quad] "+s"(quad),
        [T] "+v"(p.T), [c0] "+v"(p.c0), [c1] "+v"(p.c1), [c2] "+v"(p.c2), [c3] "+v"(p.c3)
      : [q0] "v"(q0), [q1] "v"(q1), [q2] "v"(q2), [x] "v"(pp.x), [y] "v"(pp.y), [xx] "v"(pp.xx), [xy] "v"(pp.xy), [yy] "v"(pp.yy),
        [A] "v"(A), [B] "v"(B), [C] "v"(C), [f0] "v"(f0), [f1] "v"(f1), [f2] "v"(f2), [f3] "v"(f3), [amin] "s"(amin),
        [tstop] "s"(tstop), [at] "s"(at)
      : "vcc", "scc");
}

// ---- form B: the four bodies of an entry in one block, EXEC restored once -------------------------------------------
#define BODY_B(k)                                                   \
  "s_bitcmp1_b64 %[quad" #k "], %[at]\n"                            \
  "s_cbranch_scc0 .Lnextb" #k "_%=\n"                               \
  "s_mov_b64 exec, %[alive" #k "]\n"                                \
  "v_fma_f32 %[t1], %[q1], %[x" #k "], %[q0]\n"                     \
  "v_fmac_f32 %[t1], %[q2], %[y" #k "]\n"                           \
  "v_fmac_f32 %[t1], %[A], %[xx" #k "]\n"                           \
  "v_fmac_f32 %[t1], %[B], %[xy" #k "]\n"                           \
  "v_fmac_f32 %[t1], %[C], %[yy" #k "]\n"                           \
  "v_exp_f32 %[t1], %[t1]\n"                                        \
  "s_nop 0\n"                                                       \
  "v_cmpx_le_f32 vcc, %[amin], %[t1]\n"                             \
  "v_fma_f32 %[t0], -%[t1], %[T" #k "], %[T" #k "]\n"               \
  "v_mul_f32 %[dx], %[t1], %[T" #k "]\n"                            \
  "v_cmpx_lt_f32_e64 exec, %[tstop], %[t0]\n"                       \
  "v_mov_b32 %[T" #k "], %[t0]\n"                                   \
  "v_fmac_f32 %[c0" #k "], %[dx], %[f0]\n"                          \
  "v_fmac_f32 %[c1" #k "], %[dx], %[f1]\n"                          \
  "v_fmac_f32 %[c2" #k "], %[dx], %[f2]\n"                          \
  "v_fmac_f32 %[c3" #k "], %[dx], %[f3]\n"                          \
  "s_andn2_b64 vcc, vcc, exec\n"                                    \
  "s_andn2_b64 %[alive" #k "], %[alive" #k "], vcc\n"               \
  "s_cselect_b64 %[quad" #k "], %[quad" #k "], 0\n"                 \
  ".Lnextb" #k "_%=:\n"
#define OUT_B(k) [alive##k] "+s"(alive[k]), [quad##k] "+s"(quad[k]), [T##k] "+v"(st[k].T), [c0##k] "+v"(st[k].c0), \
                 [c1##k] "+v"(st[k].c1), [c2##k] "+v"(st[k].c2), [c3##k] "+v"(st[k].c3)
#define IN_B(k) [x##k] "v"(pq[k].x), [y##k] "v"(pq[k].y), [xx##k] "v"(pq[k].xx), [xy##k] "v"(pq[k].xy), [yy##k] "v"(pq[k].yy)
__device__ __forceinline__ void entry_b(Px* st, unsigned long long* alive, unsigned long long* quad, int at, const Poly* pq,
                                        float q0, float q1, float q2, float A, float B, float C, float f0, float f1, float f2,
                                        float f3) {
  float dx, t0, t1;
  const float amin = 1.0f / 255.0f, tstop = 1e-4f;
  asm volatile(BODY_B(0) BODY_B(1) BODY_B(2) BODY_B(3)
               "s_mov_b64 exec, -1\n"
               : [dx] "=&v"(dx), [t0] "=&v"(t0), [t1] "=&v"(t1), OUT_B(0), OUT_B(1), OUT_B(2), OUT_B(3)
               : [q0] "v"(q0), [q1] "v"(q1), [q2] "v"(q2), [A] "v"(A), [B] "v"(B), [C] "v"(C), [f0] "v"(f0), [f1] "v"(f1),
                 [f2] "v"(f2), [f3] "v"(f3), [amin] "s"(amin), [tstop] "s"(tstop), [at] "s"(at), IN_B(0), IN_B(1), IN_B(2), IN_B(3)
               : "vcc", "scc");
}

// ---- form C: four form-A bodies in one block (each restores EXEC itself) ------------------------------------------
// Between two asm statements that share a register the compiler pads one wait state (`s_nop 0`, its fixed boundary
// pad): four statements per entry are four such slots, taken or skipped.  One block per entry pays one.
#define BODY_C(k)                                                   \
  "s_bitcmp1_b64 %[quad" #k "], %[at]\n"                            \
  "s_cbranch_scc0 .Lnextc" #k "_%=\n"                               \
  "v_fma_f32 %[t1], %[q1], %[x" #k "], %[q0]\n"                     \
  "v_fmac_f32 %[t1], %[q2], %[y" #k "]\n"                           \
  "v_fmac_f32 %[t1], %[A], %[xx" #k "]\n"                           \
  "v_fmac_f32 %[t1], %[B], %[xy" #k "]\n"                           \
  "v_fmac_f32 %[t1], %[C], %[yy" #k "]\n"                           \
  "v_exp_f32 %[t1], %[t1]\n"                                        \
  "s_mov_b64 exec, %[alive" #k "]\n"                                \
  "v_cmpx_le_f32 vcc, %[amin], %[t1]\n"                             \
  "v_fma_f32 %[t0], -%[t1], %[T" #k "], %[T" #k "]\n"               \
  "v_mul_f32 %[dx], %[t1], %[T" #k "]\n"                            \
  "v_cmpx_lt_f32_e64 exec, %[tstop], %[t0]\n"                       \
  "v_mov_b32 %[T" #k "], %[t0]\n"                                   \
  "v_fmac_f32 %[c0" #k "], %[dx], %[f0]\n"                          \
  "v_fmac_f32 %[c1" #k "], %[dx], %[f1]\n"                          \
  "v_fmac_f32 %[c2" #k "], %[dx], %[f2]\n"                          \
  "v_fmac_f32 %[c3" #k "], %[dx], %[f3]\n"                          \
  "s_andn2_b64 vcc, vcc, exec\n"                                    \
  "s_andn2_b64 %[alive" #k "], %[alive" #k "], vcc\n"               \
  "s_cselect_b64 %[quad" #k "], %[quad" #k "], 0\n"                 \
  "s_mov_b64 exec, -1\n"                                            \
  ".Lnextc" #k "_%=:\n"
__device__ __forceinline__ void entry_c(Px* st, unsigned long long* alive, unsigned long long* quad, int at, const Poly* pq,
                                        float q0, float q1, float q2, float A, float B, float C, float f0, float f1, float f2,
                                        float f3) {
  float dx, t0, t1;
  const float amin = 1.0f / 255.0f, tstop = 1e-4f;
  asm volatile(BODY_C(0) BODY_C(1) BODY_C(2) BODY_C(3)
               : [dx] "=&v"(dx), [t0] "=&v"(t0), [t1] "=&v"(t1), OUT_B(0), OUT_B(1), OUT_B(2), OUT_B(3)
               : [q0] "v"(q0), [q1] "v"(q1), [q2] "v"(q2), [A] "v"(A), [B] "v"(B), [C] "v"(C), [f0] "v"(f0), [f1] "v"(f1),
                 [f2] "v"(f2), [f3] "v"(f3), [amin] "s"(amin), [tstop] "s"(tstop), [at] "s"(at), IN_B(0), IN_B(1), IN_B(2), IN_B(3)
               : "vcc", "scc");
}

struct Entry { float q0, q1, q2, A, B, C; unsigned mask; int idx; float f0, f1, f2, f3; float pad[4]; };   // 64 bytes

// synthetic entry of batch b for queue position j (queue_feed.hip: exponent in [-9, 0] so that ~40 % of the lanes pass
// alpha >= 1/255 with opacity ~0.5, quadrant sets with 2.25 members on average)
__device__ __forceinline__ Entry make_entry(unsigned b, unsigned j, unsigned seed) {
  unsigned h = (b * 64u + j) * 2654435761u + seed * 40503u;
  h ^= h >> 15; h *= 2246822519u; h ^= h >> 13;
  Entry e;
  const float u0 = (float)(h & 1023u) / 1023.f, u1 = (float)((h >> 10) & 1023u) / 1023.f, u2 = (float)((h >> 20) & 1023u) / 1023.f;
  e.A = -0.02f - 0.05f * u0; e.C = -0.02f - 0.05f * u1; e.B = 0.02f * (u2 - 0.5f);
  const float mx = 14.f * (u1 - 0.5f), my = 14.f * (u2 - 0.5f);
  e.q0 = e.A * mx * mx + e.B * mx * my + e.C * my * my - 1.2f;
  e.q1 = -(2.f * e.A * mx + e.B * my);
  e.q2 = -(2.f * e.C * my + e.B * mx);
  const unsigned r = (h >> 7) & 15u;
  const unsigned masks[16] = {1, 2, 4, 8, 3, 12, 5, 10, 3, 12, 7, 11, 13, 14, 15, 15};
  e.mask = masks[r];
  e.idx = (int)(b * 64u + j);
  e.f0 = u0; e.f1 = u1; e.f2 = u2; e.f3 = 7.f + u0;
  e.pad[0] = e.pad[1] = e.pad[2] = e.pad[3] = 0.f;
  return e;
}

// out: 5 floats per pixel (T and the four colours) so that the forms can be compared bit for bit; emptied[wave]: how
// often a quadrant's last pixel closed inside a batch (the bodies after it are skipped: the host's body count assumes none)
template <int FORM>
__global__ __launch_bounds__(64, 8) void walk_kernel(float* out, unsigned long long* times, unsigned* emptied, int n_batches, int count,
                                                    unsigned seed) {
  extern __shared__ unsigned char pad_[];
  __shared__ Entry queue[65];
  const unsigned lane = threadIdx.x & 63u;
  Poly pq[4];
  Px st[4];
  unsigned long long alive[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float x = (float)(lane & 7) - 7.5f + 8.f * (k & 1), y = (float)(lane >> 3) - 7.5f + 8.f * (k >> 1);
    pq[k] = Poly{x, y, x * x, x * y, y * y};
    st[k] = Px{1.f, 0.f, 0.f, 0.f, 0.f};
    alive[k] = ~0ull;
  }
  unsigned n_emptied = 0;
  const unsigned long long t0 = __builtin_amdgcn_s_memtime(), r0 = __builtin_amdgcn_s_memrealtime();
  for (int b = 0; b < n_batches; ++b) {
    // each lane queues its own entry; the quadrant sets become four lane masks, as the cull leaves them
    const bool queued = (int)lane < count;
    const Entry mine = make_entry((unsigned)b + blockIdx.x * 977u, lane, seed);
    unsigned long long reach[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) reach[k] = __ballot(queued && ((mine.mask >> k) & 1u));
    const unsigned long long keep = __ballot(queued);
    if (queued) queue[lane] = mine;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    unsigned long long rest = keep;
    for (const Entry* q = queue; rest != 0ull; ++q) {
      const int at = __builtin_ctzll(rest);
      asm("s_bitset0_b64 %0, %1" : "+s"(rest) : "s"(at));
      const f4* e = reinterpret_cast<const f4*>(q);
      f4 g0 = e[0], g1 = e[1], g2 = e[2];
      asm volatile("" : "+v"(g0), "+v"(g1), "+v"(g2));
      if constexpr (FORM == 2) {
        entry_b(st, alive, reach, at, pq, g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, g2.x, g2.y, g2.z, g2.w);
      } else if constexpr (FORM == 3) {
        entry_c(st, alive, reach, at, pq, g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, g2.x, g2.y, g2.z, g2.w);
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          if constexpr (FORM == 0) body_0(st[k], alive[k], reach[k], at, pq[k], g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, g2.x, g2.y, g2.z, g2.w);
          else body_a(st[k], alive[k], reach[k], at, pq[k], g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, g2.x, g2.y, g2.z, g2.w);
        }
      }
    }
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      n_emptied += alive[k] == 0ull;
      alive[k] = ~0ull;                                        // keep the pixels open: constant work per body
      st[k].T = st[k].T < 0.05f ? 1.f : st[k].T;
    }
  }
  const unsigned long long t1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
  if (lane == 0) { times[2 * blockIdx.x] = t1 - t0; times[2 * blockIdx.x + 1] = r1 - r0; emptied[blockIdx.x] = n_emptied; }
  float* o = out + ((size_t)blockIdx.x * 64 + lane) * 20;
#pragma unroll
  for (int k = 0; k < 4; ++k) { o[5 * k] = st[k].T; o[5 * k + 1] = st[k].c0; o[5 * k + 2] = st[k].c1; o[5 * k + 3] = st[k].c2; o[5 * k + 4] = st[k].c3; }
}

static double median(std::vector<double> v) { std::sort(v.begin(), v.end()); return v[v.size() / 2]; }

int main(int argc, char** argv) {
  const int n_batches = argc > 1 ? atoi(argv[1]) : 48, count = argc > 2 ? atoi(argv[2]) : 54, rounds = argc > 3 ? atoi(argv[3]) : 10;
  setvbuf(stdout, nullptr, _IONBF, 0);
  if (n_batches < 1 || count < 1 || count > 64 || rounds < 3) { printf("usage: [batches >= 1] [queued entries 1..64] [rounds >= 3]\n"); return 1; }
  hipDeviceProp_t prop;
  CHECK(hipGetDeviceProperties(&prop, 0));
  const int cus = prop.multiProcessorCount;
  printf("device %s, %d CUs; %d batches of %d queued entries per wave, 2.25 quadrant bodies per entry; %d rounds, the first dropped\n",
         prop.gcnArchName, cus, n_batches, count, rounds);
  const double bodies = (double)n_batches * count * 36.0 / 16.0;      // host replica of the mask table, all quadrants live
  constexpr int kForms = 4;
  const void* fns[kForms] = {(const void*)walk_kernel<0>, (const void*)walk_kernel<1>, (const void*)walk_kernel<2>, (const void*)walk_kernel<3>};
  const char* names[kForms] = {"0: shipped body, 7 scalar slots", "A: s_mov in the wait state, 5 slots", "B: one block per entry, 5 + 1/entry",
                               "C: form A bodies, one block per entry"};
  for (const void* fn : fns) CHECK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 8192));
  hipEvent_t e0, e1;
  CHECK(hipEventCreate(&e0)); CHECK(hipEventCreate(&e1));
  double cyc_at[kForms][9] = {};
  printf("%-38s %6s %8s | %9s %9s | %12s %8s | %8s %8s | %5s %s\n", "form", "w/SIMD", "waves", "launch us", "min", "ns/body/wave", "min",
         "cyc/VALU", "min", "GHz", "pixels == form 0");
  for (int wps : {4, 5, 6, 8}) {
    const int per_cu = 4 * wps, waves = cus * per_cu * 3;             // the launch holds three times the resident waves
    float* out; unsigned long long* times; unsigned* emptied;
    const size_t out_floats = (size_t)waves * 64 * 20;
    CHECK(hipMalloc(&out, out_floats * 4));
    CHECK(hipMalloc(&times, (size_t)waves * 16));
    CHECK(hipMalloc(&emptied, (size_t)waves * 4));
    int dyn[kForms]; double wps_real[kForms];
    for (int f = 0; f < kForms; ++f) {
      // the largest dynamic LDS footprint with which the occupancy API still reports per_cu one-wave workgroups per CU
      int d = 160 * 1024 / per_cu / 256 * 256, fit = 0;
      for (; d >= 0; d -= 256) {
        CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&fit, fns[f], 64, d));
        if (fit >= per_cu) break;
      }
      dyn[f] = d < 0 ? 0 : d;
      wps_real[f] = fit / 4.0;
    }
    std::vector<double> us[kForms], ns[kForms], cyc[kForms];
    double ghz[kForms] = {};
    bool same[kForms] = {true, true, true, true};
    unsigned long long n_emptied = 0;
    std::vector<float> ref(out_floats), got(out_floats);
    std::vector<unsigned long long> t((size_t)waves * 2);
    std::vector<unsigned> em(waves);
    for (int round = 0; round < rounds; ++round) {
      for (int i = 0; i < kForms; ++i) {
        const int f = (i + round) % kForms;
        const unsigned seed = 7u;                                     // one seed: every launch computes the same pixels
        CHECK(hipEventRecord(e0));
        if (f == 0) hipLaunchKernelGGL(walk_kernel<0>, dim3(waves), dim3(64), dyn[f], 0, out, times, emptied, n_batches, count, seed);
        else if (f == 1) hipLaunchKernelGGL(walk_kernel<1>, dim3(waves), dim3(64), dyn[f], 0, out, times, emptied, n_batches, count, seed);
        else if (f == 2) hipLaunchKernelGGL(walk_kernel<2>, dim3(waves), dim3(64), dyn[f], 0, out, times, emptied, n_batches, count, seed);
        else hipLaunchKernelGGL(walk_kernel<3>, dim3(waves), dim3(64), dyn[f], 0, out, times, emptied, n_batches, count, seed);
        CHECK(hipGetLastError());
        CHECK(hipEventRecord(e1));
        CHECK(hipEventSynchronize(e1));
        float ms;
        CHECK(hipEventElapsedTime(&ms, e0, e1));
        CHECK(hipMemcpy(t.data(), times, (size_t)waves * 16, hipMemcpyDeviceToHost));
        if (round == 0) {
          CHECK(hipMemcpy(f == 0 ? ref.data() : got.data(), out, out_floats * 4, hipMemcpyDeviceToHost));
          if (f == 0) {
            CHECK(hipMemcpy(em.data(), emptied, (size_t)waves * 4, hipMemcpyDeviceToHost));
            for (unsigned v : em) n_emptied += v;
          }
          continue;                                                   // (round 0 runs form 0 first: ref is filled before it is read)
        }
        if (round == 1 && f != 0) {
          CHECK(hipMemcpy(got.data(), out, out_floats * 4, hipMemcpyDeviceToHost));
          same[f] = memcmp(ref.data(), got.data(), out_floats * 4) == 0;
        }
        double sc = 0, rc = 0;
        for (int w = 0; w < waves; ++w) { sc += (double)t[2 * w]; rc += (double)t[2 * w + 1]; }
        ghz[f] = sc / rc * 0.1;                                       // shader cycles per 10 ns tick
        us[f].push_back(ms * 1e3);
        ns[f].push_back(rc / waves * 10.0 / bodies);
        // SIMD-cycles per vector instruction: the wave's shader cycles / (its 15 per body x the waves sharing the SIMD)
        cyc[f].push_back((sc / waves) / (bodies * 15 * wps_real[f]));
      }
    }
    for (int f = 0; f < kForms; ++f) {
      cyc_at[f][wps] = median(cyc[f]);
      printf("%-38s %6.2f %8d | %9.1f %9.1f | %12.2f %8.2f | %8.3f %8.3f | %5.2f %s\n", names[f], wps_real[f], waves, median(us[f]),
             *std::min_element(us[f].begin(), us[f].end()), median(ns[f]), *std::min_element(ns[f].begin(), ns[f].end()), median(cyc[f]),
             *std::min_element(cyc[f].begin(), cyc[f].end()), ghz[f], f == 0 ? "-" : same[f] ? "identical" : "DIFFERENT");
    }
    printf("  (quadrants whose last pixel closed inside a batch, all waves of one launch: %llu)\n", n_emptied);
    CHECK(hipFree(out)); CHECK(hipFree(times)); CHECK(hipFree(emptied));
  }
  // the gate: a form goes on only if it does not price higher than form 0 at 5 AND at 8 waves per SIMD
  for (int f = 1; f < kForms; ++f)
    printf("form %c against form 0, median SIMD-cycles per vector instruction: %.3f vs %.3f at 5 waves, %.3f vs %.3f at 8 waves: %s\n",
           "0ABC"[f], cyc_at[f][5], cyc_at[0][5], cyc_at[f][8], cyc_at[0][8],
           cyc_at[f][5] <= cyc_at[0][5] && cyc_at[f][8] <= cyc_at[0][8] ? "not higher" : "HIGHER");
  return 0;
}
