// csrc/launch_plan.cuh for the 8-byte scalars of lasso_hyrax_commit_compressed_u64 (include/lasso_hip_poly.h): whatever the switches and tables, msm_plan names the bucket
// kernel; its work units count W nibbles, not a full-width scalar; its chunks cover the columns and never outnumber what msm_pts_bytes reserves.  (The plan's answers for 4
// and 32 bytes are walked by tests/cpp/test_launch_plan_host.cpp.)
#include "../../lasso_amd/csrc/launch_plan.cuh"
#include <cstdio>
#define CHECK(c) do { if (!(c)) { printf("FAIL %s line %d\n", #c, __LINE__); return 1; } } while (0)

int main() {
  const size_t ROWS[] = {1, 3, 16, 17, 32, 33, 255, 256, 1024, 4096}, COLS[] = {1, 2, 255, 511, 512, 4096, 16384};
  for (size_t rows : ROWS) for (size_t cols : COLS) for (uint32_t W = 9; W <= 16; W++) for (int bools = 0; bools < 64; bools++) for (int comp = 0; comp < 2; comp++) {
    const MsmSwitches sw = {(bools & 1) != 0, (bools & 2) != 0, (bools & 4) != 0, (bools & 8) != 0, (bools & 16) != 0, 0, 512, 1200, 0};
    const MsmHave have = {16386, (bools & 32) != 0, (bools & 32) != 0, true, true};
    const MsmShape s = {8, W, rows, cols, comp != 0, false};
    const MsmPlan p = msm_plan(s, have, sw);
    CHECK(p.kernel == MSM_K_BUCKETS);
    CHECK(p.pip_group == 0);
    CHECK(p.ref_adds == msm_ref_adds(rows, cols, 4 * W));
    CHECK(p.adds == (double)rows * cols * W);
    CHECK(p.K >= 1 && p.K * p.cols_per_chunk >= cols && (p.K - 1) * p.cols_per_chunk < cols);
    CHECK(p.K == msm_chunks(rows, cols, W) && p.K <= msm_chunks(rows, cols, MSM_WINDOWS));       // msm_pts_bytes reserves for 64 windows
    CHECK(msm_pts_bytes(rows, cols, 256) >= (rows * p.K + 2 * rows) * MSM_PT29_BYTES + 512);
    const MsmShape s4 = {4, 8, rows, cols, comp != 0, false};
    CHECK(msm_plan(s4, have, sw).ref_adds == msm_ref_adds(rows, cols, 32));
    const MsmShape s32 = {32, MSM_WINDOWS, rows, cols, comp != 0, false};
    const MsmPlan p32 = msm_plan(s32, have, sw);
    if (p32.kernel != MSM_K_DIRECT) CHECK(p32.ref_adds == msm_ref_adds(rows, cols, FR_MODULUS_BITS));
  }
  printf("OK\n");
  return 0;
}
