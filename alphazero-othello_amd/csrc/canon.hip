// canon.hip — positions and their rows up to the eight symmetries of the square
// (oth_canon_*, az_rows_d4_*, az_rows_symmetrise_*; include/az_othello.h has the contract).
//
// The arithmetic is bitboard.h's (canon, d4_square_a, orbit_min, symmetrise_one), the same
// code on both sides, so the host and device entry points agree bit for bit.
//   * k_canon2: two consecutive positions per lane, every access a lane-contiguous 16-byte
//     (boards) or 2-byte (sym / stab) one, as k_step2; needs 16-byte aligned board arrays and
//     2-byte aligned byte arrays.  k_canon1: one position per lane, any alignment.  The
//     entry point picks by the pointers.  No LDS, no scratch: the sixteen images live in
//     registers (d4_images is indexed by constants only).
//   * k_rows_d4 / k_rows_sym: one wavefront per 65-float row, lane = destination square; the
//     row is read coalesced, each lane fetches its source value from the lane that holds it
//     with __shfl, and the row is written coalesced.  Lane 0 carries the pass entry.
//   * k_act_d4: the rows' actions, one per lane.
// Every kernel is one plain launch on the caller's stream: no allocation, no
// synchronisation, nothing that a stream capture could not record.
#include "bitboard.h"
#include "common.h"

namespace {

constexpr int kBlock = 256;
constexpr int kWave = 64;
constexpr unsigned kGridCap = 256 * 64;

typedef uint64_t u64x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

struct CanonOut {
  uint64_t own, opp;
  uint8_t sym, stab;
};

// canon() with the contract's error row: overlapping boards pass through, sym = 255, stab = 0
AZ_HD CanonOut canon_row(uint64_t own, uint64_t opp) {
  const azb::Canon c = azb::canon(own, opp);
  const bool bad = (own & opp) != 0;
  return CanonOut{bad ? own : c.own, bad ? opp : c.opp, (uint8_t)(bad ? AZ_CANON_BAD : c.sym),
                  (uint8_t)(bad ? 0 : c.stab)};
}

// an action under a row's symmetry, then the smallest square of its orbit; the pass stays,
// a sym above 7 or an action above 64 gives AZ_CANON_BAD
AZ_HD uint8_t act_row(int a, int sym, int stab) {
  if (sym > 7 || a > azb::kPass) return (uint8_t)AZ_CANON_BAD;
  if (a == azb::kPass) return (uint8_t)a;
  return (uint8_t)azb::orbit_min(azb::d4_square_a(a, sym), stab);
}

__device__ __forceinline__ float quiet_nan() { return __builtin_nanf(""); }

__global__ __launch_bounds__(kBlock) void k_canon1(const uint64_t* __restrict__ own,
                                                   const uint64_t* __restrict__ opp, int64_t n,
                                                   uint64_t* __restrict__ own_o,
                                                   uint64_t* __restrict__ opp_o,
                                                   uint8_t* __restrict__ sym_o,
                                                   uint8_t* __restrict__ stab_o) {
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
    const CanonOut c = canon_row(own[i], opp[i]);
    own_o[i] = c.own;
    opp_o[i] = c.opp;
    sym_o[i] = c.sym;
    stab_o[i] = c.stab;
  }
}

__global__ __launch_bounds__(kBlock) void k_canon2(const uint64_t* __restrict__ own,
                                                   const uint64_t* __restrict__ opp, int64_t n,
                                                   uint64_t* __restrict__ own_o,
                                                   uint64_t* __restrict__ opp_o,
                                                   uint8_t* __restrict__ sym_o,
                                                   uint8_t* __restrict__ stab_o) {
  const int64_t pairs = (n + 1) / 2, full = n / 2;
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x; j < pairs; j += stride) {
    if (j < full) {
      const u64x2 a = __builtin_nontemporal_load(reinterpret_cast<const u64x2*>(own) + j);
      const u64x2 b = __builtin_nontemporal_load(reinterpret_cast<const u64x2*>(opp) + j);
      const CanonOut c0 = canon_row(a.x, b.x), c1 = canon_row(a.y, b.y);
      const u64x2 vo = {c0.own, c1.own}, vp = {c0.opp, c1.opp};
      __builtin_nontemporal_store(vo, reinterpret_cast<u64x2*>(own_o) + j);
      __builtin_nontemporal_store(vp, reinterpret_cast<u64x2*>(opp_o) + j);
      reinterpret_cast<uint16_t*>(sym_o)[j] = (uint16_t)(c0.sym | (c1.sym << 8));
      reinterpret_cast<uint16_t*>(stab_o)[j] = (uint16_t)(c0.stab | (c1.stab << 8));
    } else {  // odd n: the last position alone
      const int64_t i = 2 * j;
      const CanonOut c = canon_row(own[i], opp[i]);
      own_o[i] = c.own;
      opp_o[i] = c.opp;
      sym_o[i] = c.sym;
      stab_o[i] = c.stab;
    }
  }
}

__global__ __launch_bounds__(kBlock) void k_act_d4(const uint8_t* __restrict__ act,
                                                   const uint8_t* __restrict__ sym,
                                                   const uint8_t* __restrict__ stab, int64_t n,
                                                   uint8_t* __restrict__ act_o) {
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride)
    act_o[i] = act_row(act[i], sym[i], stab ? stab[i] : 1);
}

// pi_o[d4_square_a(j, sym)] = pi[j]: lane d holds pi[d] and takes pi[d4_square_inv(d, sym)]
__global__ __launch_bounds__(kBlock) void k_rows_d4(const float* __restrict__ pi,
                                                    const uint8_t* __restrict__ sym, int64_t n,
                                                    float* __restrict__ pi_o) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t waves = (int64_t)gridDim.x * (kBlock / kWave);
  for (int64_t r = (int64_t)blockIdx.x * (kBlock / kWave) + threadIdx.x / kWave; r < n;
       r += waves) {
    const float* row = pi + r * 65;
    float* out = pi_o + r * 65;
    const int s = sym[r];
    const float v = row[lane];
    const float w = __shfl(v, azb::d4_square_inv(lane, s & 7), kWave);
    const bool bad = s > 7;
    out[lane] = bad ? quiet_nan() : w;
    if (lane == 0) out[64] = bad ? quiet_nan() : row[64];
  }
}

__global__ __launch_bounds__(kBlock) void k_rows_sym(const float* __restrict__ pi,
                                                     const uint8_t* __restrict__ stab, int64_t n,
                                                     float* __restrict__ pi_o) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t waves = (int64_t)gridDim.x * (kBlock / kWave);
  for (int64_t r = (int64_t)blockIdx.x * (kBlock / kWave) + threadIdx.x / kWave; r < n;
       r += waves) {
    const float* row = pi + r * 65;
    float* out = pi_o + r * 65;
    const int st = stab[r];
    const float x = row[lane];
    float v[8];
#pragma unroll
    for (int t = 0; t < 8; ++t) v[t] = __shfl(x, azb::d4_square_inv(lane, t), kWave);
    const bool bad = st == 0;
    out[lane] = bad ? quiet_nan() : azb::symmetrise_one(v, st);
    if (lane == 0) out[64] = bad ? quiet_nan() : row[64];
  }
}

// A float4 copy on k_canon2's grid: the yardstick the canon figures are read against
// (scripts/bench_canon.py measures both in one run).  A measurement probe only.
__global__ __launch_bounds__(kBlock) void k_copy16(const f32x4* __restrict__ src,
                                                   f32x4* __restrict__ dst, int64_t n16) {
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n16; i += stride)
    __builtin_nontemporal_store(__builtin_nontemporal_load(src + i), dst + i);
}

unsigned grid_for(int64_t items, int per_block) {
  const int64_t g = (items + per_block - 1) / per_block;
  return (unsigned)(g < 1 ? 1 : (g > (int64_t)kGridCap ? (int64_t)kGridCap : g));
}

bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

int canon_args(const char* who, const uint64_t* own, const uint64_t* opp, int64_t n,
               uint64_t* own_o, uint64_t* opp_o, uint8_t* sym_o, uint8_t* stab_o) {
  AZ_REQUIRE(n >= 0, AZ_ERR_ARG, "%s: n=%lld < 0", who, (long long)n);
  AZ_REQUIRE(n == 0 || (own && opp && own_o && opp_o && sym_o && stab_o), AZ_ERR_ARG,
             "%s: null buffer", who);
  return AZ_OK;
}

int rows_args(const char* who, const float* pi, const uint8_t* act, const uint8_t* sym,
              int64_t n, float* pi_o, uint8_t* act_o) {
  AZ_REQUIRE(n >= 0, AZ_ERR_ARG, "%s: n=%lld < 0", who, (long long)n);
  AZ_REQUIRE((pi == nullptr) == (pi_o == nullptr) && (act == nullptr) == (act_o == nullptr),
             AZ_ERR_ARG, "%s: pi / pi_o and act / act_o must be given or NULL together", who);
  AZ_REQUIRE(n == 0 || !pi || pi != pi_o, AZ_ERR_ARG, "%s: pi_o must not be pi", who);
  AZ_REQUIRE(n == 0 || sym, AZ_ERR_ARG, "%s: null sym", who);
  return AZ_OK;
}

int sym_args(const char* who, const float* pi, const uint8_t* stab, int64_t n, float* pi_o) {
  AZ_REQUIRE(n >= 0, AZ_ERR_ARG, "%s: n=%lld < 0", who, (long long)n);
  AZ_REQUIRE(n == 0 || (pi && stab && pi_o), AZ_ERR_ARG, "%s: null buffer", who);
  AZ_REQUIRE(n == 0 || pi != pi_o, AZ_ERR_ARG, "%s: pi_o must not be pi", who);
  return AZ_OK;
}

}  // namespace

extern "C" {

int oth_canon_cpu(const uint64_t* own, const uint64_t* opp, int64_t n, uint64_t* own_o,
                  uint64_t* opp_o, uint8_t* sym_o, uint8_t* stab_o) {
  const int rc = canon_args("oth_canon_cpu", own, opp, n, own_o, opp_o, sym_o, stab_o);
  if (rc != AZ_OK) return rc;
  for (int64_t i = 0; i < n; ++i) {
    const CanonOut c = canon_row(own[i], opp[i]);
    own_o[i] = c.own;
    opp_o[i] = c.opp;
    sym_o[i] = c.sym;
    stab_o[i] = c.stab;
  }
  return AZ_OK;
}

int oth_canon_gpu(const uint64_t* own, const uint64_t* opp, int64_t n, uint64_t* own_o,
                  uint64_t* opp_o, uint8_t* sym_o, uint8_t* stab_o, void* stream) {
  const int rc = canon_args("oth_canon_gpu", own, opp, n, own_o, opp_o, sym_o, stab_o);
  if (rc != AZ_OK) return rc;
  if (n == 0) return AZ_OK;
  const bool wide = aligned(own, 16) && aligned(opp, 16) && aligned(own_o, 16) &&
                    aligned(opp_o, 16) && aligned(sym_o, 2) && aligned(stab_o, 2);
  if (wide)
    hipLaunchKernelGGL(k_canon2, dim3(grid_for((n + 1) / 2, kBlock)), dim3(kBlock), 0,
                       azc::as_stream(stream), own, opp, n, own_o, opp_o, sym_o, stab_o);
  else
    hipLaunchKernelGGL(k_canon1, dim3(grid_for(n, kBlock)), dim3(kBlock), 0,
                       azc::as_stream(stream), own, opp, n, own_o, opp_o, sym_o, stab_o);
  AZ_HIP(hipGetLastError());
  return AZ_OK;
}

int az_copy16_probe_gpu(const void* src, void* dst, int64_t n16, void* stream) {
  AZ_REQUIRE(n16 >= 0, AZ_ERR_ARG, "az_copy16_probe_gpu: n16 < 0");
  if (n16 == 0) return AZ_OK;
  AZ_REQUIRE(src && dst && src != dst && aligned(src, 16) && aligned(dst, 16), AZ_ERR_ARG,
             "az_copy16_probe_gpu: needs two distinct 16-byte aligned buffers");
  hipLaunchKernelGGL(k_copy16, dim3(grid_for(n16, kBlock)), dim3(kBlock), 0,
                     azc::as_stream(stream), static_cast<const f32x4*>(src),
                     static_cast<f32x4*>(dst), n16);
  AZ_HIP(hipGetLastError());
  return AZ_OK;
}

int az_rows_d4_cpu(const float* pi, const uint8_t* act, const uint8_t* sym, const uint8_t* stab,
                   int64_t n, float* pi_o, uint8_t* act_o) {
  const int rc = rows_args("az_rows_d4_cpu", pi, act, sym, n, pi_o, act_o);
  if (rc != AZ_OK) return rc;
  for (int64_t r = 0; r < n; ++r) {
    const int s = sym[r];
    if (pi) {
      const float* row = pi + r * 65;
      float* out = pi_o + r * 65;
      for (int d = 0; d < 64; ++d)
        out[d] = s > 7 ? __builtin_nanf("") : row[azb::d4_square_inv(d, s)];
      out[64] = s > 7 ? __builtin_nanf("") : row[64];
    }
    if (act) act_o[r] = act_row(act[r], s, stab ? stab[r] : 1);
  }
  return AZ_OK;
}

int az_rows_d4_gpu(const float* pi, const uint8_t* act, const uint8_t* sym, const uint8_t* stab,
                   int64_t n, float* pi_o, uint8_t* act_o, void* stream) {
  const int rc = rows_args("az_rows_d4_gpu", pi, act, sym, n, pi_o, act_o);
  if (rc != AZ_OK) return rc;
  if (n == 0) return AZ_OK;
  if (pi) {
    hipLaunchKernelGGL(k_rows_d4, dim3(grid_for(n, kBlock / kWave)), dim3(kBlock), 0,
                       azc::as_stream(stream), pi, sym, n, pi_o);
    AZ_HIP(hipGetLastError());
  }
  if (act) {
    hipLaunchKernelGGL(k_act_d4, dim3(grid_for(n, kBlock)), dim3(kBlock), 0,
                       azc::as_stream(stream), act, sym, stab, n, act_o);
    AZ_HIP(hipGetLastError());
  }
  return AZ_OK;
}

int az_rows_symmetrise_cpu(const float* pi, const uint8_t* stab, int64_t n, float* pi_o) {
  const int rc = sym_args("az_rows_symmetrise_cpu", pi, stab, n, pi_o);
  if (rc != AZ_OK) return rc;
  for (int64_t r = 0; r < n; ++r) {
    const float* row = pi + r * 65;
    float* out = pi_o + r * 65;
    const int st = stab[r];
    for (int d = 0; d < 64; ++d) {
      float v[8];
      for (int t = 0; t < 8; ++t) v[t] = row[azb::d4_square_inv(d, t)];
      out[d] = st == 0 ? __builtin_nanf("") : azb::symmetrise_one(v, st);
    }
    out[64] = st == 0 ? __builtin_nanf("") : row[64];
  }
  return AZ_OK;
}

int az_rows_symmetrise_gpu(const float* pi, const uint8_t* stab, int64_t n, float* pi_o,
                           void* stream) {
  const int rc = sym_args("az_rows_symmetrise_gpu", pi, stab, n, pi_o);
  if (rc != AZ_OK) return rc;
  if (n == 0) return AZ_OK;
  hipLaunchKernelGGL(k_rows_sym, dim3(grid_for(n, kBlock / kWave)), dim3(kBlock), 0,
                     azc::as_stream(stream), pi, stab, n, pi_o);
  AZ_HIP(hipGetLastError());
  return AZ_OK;
}

}  // extern "C"
