// rng_probe.hip — test support: the engine's device random draws, as arrays.
//
// az_rng_uniform_* return azr::uniform2 for a run of slots at one (event, sub-draw, stream);
// az_rng_dirichlet_gpu returns what k_expand's root expansion draws for (slot, event): the 65
// raw gammas and the normalised vector, from the same azr::dirichlet65 the engine calls.
// Nothing here restates the sampler; the tests compare these arrays with references of their
// own (tests/test_rng_cpu.py, tests/test_rng_gpu.py).
#include "common.h"
#include "philox.h"

namespace {

constexpr int kBlock = 256;

__global__ __launch_bounds__(kBlock) void k_rng_uniform(uint64_t seed, uint32_t stream,
                                                        uint32_t slot0, int64_t n, uint32_t event,
                                                        uint32_t sub, double* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  double a, b;
  azr::uniform2(seed, slot0 + (uint32_t)i, event, sub, stream, &a, &b);
  out[2 * i] = a;
  out[2 * i + 1] = b;
}

// one wavefront per slot, as in k_expand
__global__ __launch_bounds__(64) void k_rng_dirichlet(uint64_t seed, uint32_t stream,
                                                      uint32_t slot0, uint32_t event, double alpha,
                                                      double* __restrict__ gammas,
                                                      double* __restrict__ noise) {
  const int64_t i = blockIdx.x;
  const uint32_t lane = threadIdx.x;
  const azr::Dirichlet65 d =
      azr::dirichlet65(alpha, seed, slot0 + (uint32_t)i, event, lane, stream);
  gammas[i * 65 + lane] = d.ga;
  noise[i * 65 + lane] = d.n;
  if (lane == 0) {
    gammas[i * 65 + 64] = d.ga64;
    noise[i * 65 + 64] = d.n64;
  }
}

}  // namespace

extern "C" {

int az_rng_uniform_cpu(uint64_t seed, uint32_t stream_id, uint32_t slot0, int64_t n,
                       uint32_t event, uint32_t sub, double* out) {
  AZ_REQUIRE(n >= 0, AZ_ERR_ARG, "az_rng_uniform_cpu: n=%lld < 0", (long long)n);
  if (n == 0) return AZ_OK;
  AZ_REQUIRE(out, AZ_ERR_ARG, "az_rng_uniform_cpu: null buffer");
  for (int64_t i = 0; i < n; ++i)
    azr::uniform2(seed, slot0 + (uint32_t)i, event, sub, stream_id, &out[2 * i], &out[2 * i + 1]);
  return AZ_OK;
}

int az_rng_uniform_gpu(uint64_t seed, uint32_t stream_id, uint32_t slot0, int64_t n,
                       uint32_t event, uint32_t sub, double* out, void* stream) {
  AZ_REQUIRE(n >= 0 && n < (int64_t(1) << 31), AZ_ERR_ARG,
             "az_rng_uniform_gpu: n=%lld outside [0, 2^31)", (long long)n);
  if (n == 0) return AZ_OK;
  AZ_REQUIRE(out, AZ_ERR_ARG, "az_rng_uniform_gpu: null buffer");
  const unsigned grid = (unsigned)((n + kBlock - 1) / kBlock);
  hipLaunchKernelGGL(k_rng_uniform, dim3(grid), dim3(kBlock), 0, azc::as_stream(stream), seed,
                     stream_id, slot0, n, event, sub, out);
  AZ_HIP(hipGetLastError());
  return AZ_OK;
}

int az_rng_dirichlet_gpu(uint64_t seed, uint32_t stream_id, uint32_t slot0, int64_t n,
                         uint32_t event, double alpha, double* gammas, double* noise,
                         void* stream) {
  AZ_REQUIRE(n >= 0 && n < (int64_t(1) << 31), AZ_ERR_ARG,
             "az_rng_dirichlet_gpu: n=%lld outside [0, 2^31)", (long long)n);
  AZ_REQUIRE(alpha > 0.0, AZ_ERR_ARG, "az_rng_dirichlet_gpu: alpha=%g must be > 0", alpha);
  AZ_REQUIRE(stream_id < 0x80000000u, AZ_ERR_ARG,
             "az_rng_dirichlet_gpu: stream_id=%u must be below 2^31 (the gamma sampler's second "
             "stream is stream_id ^ 0x80000000)", (unsigned)stream_id);
  if (n == 0) return AZ_OK;
  AZ_REQUIRE(gammas && noise, AZ_ERR_ARG, "az_rng_dirichlet_gpu: null buffer");
  hipLaunchKernelGGL(k_rng_dirichlet, dim3((unsigned)n), dim3(64), 0, azc::as_stream(stream),
                     seed, stream_id, slot0, event, alpha, gammas, noise);
  AZ_HIP(hipGetLastError());
  return AZ_OK;
}

}  // extern "C"
