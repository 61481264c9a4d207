// Fragment of tests/cpp/mock_device.cpp (-DMOCK_EXT_GENS): the one entry point of include/lasso_hip_gens.h, implemented with the PRODUCT's pt_from_candidate
// (lasso_amd/csrc/fe29.cuh / bn254_fe29.cuh — the function k_points_from_candidates runs per lane) compiled for the host.  lasso_host_gens_new takes the device route on the CPU.
#include "../../lasso_amd/csrc/fe29.cuh"

extern "C" int32_t lasso_points_from_candidates(lasso_ctx* c, const uint64_t* limbs, const uint8_t* greatest, size_t n, lasso_affine* out, uint8_t* status) {
  if (!c || !status || ((!limbs || !greatest) && n)) return LASSO_ERR_INVALID;
  for (size_t i = 0; i < n; i++) {
    uint32_t in[8], aff[16];
    memcpy(in, limbs + 4 * i, 32);
    status[i] = (uint8_t)pt_from_candidate(in, greatest[i] != 0, aff);
    if (out) memcpy(&out[i], aff, 64);
  }
  return 0;
}
