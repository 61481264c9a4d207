// Fragment of tests/cpp/mock_device.cpp (-DMOCK_EXT_WIRE): the one entry point of include/lasso_hip_wire.h, implemented with the PRODUCT's pt_decompress
// (lasso_amd/csrc/fe29.cuh / bn254_fe29.cuh — the function k_points_decompress runs per lane) compiled for the host.  The verifier takes its batched path on the CPU.
#include "../../lasso_amd/csrc/fe29.cuh"

extern "C" int32_t lasso_points_decompress(lasso_ctx* c, const uint8_t* wire32, size_t n, lasso_affine* out, uint8_t* canon32, uint8_t* status) {
  if (!c || !status || (!wire32 && n)) return LASSO_ERR_INVALID;
  for (size_t i = 0; i < n; i++) {
    uint32_t in[8], aff[16], canon[8];
    memcpy(in, wire32 + 32 * i, 32);
    status[i] = (uint8_t)pt_decompress(in, aff, canon);
    if (out) memcpy(&out[i], aff, 64);
    if (canon32) memcpy(canon32 + 32 * i, canon, 32);
  }
  return 0;
}
