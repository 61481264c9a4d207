// lasso_amd/csrc/operand_layout.cuh — the text k_densify_extract_operands and the host library compile — as a stand-alone host program.
// argv[1]: a file of lines "operands chunk_bits msb_first C log_m x y" (x, y hexadecimal).  Per line: "<check> <x fits> <y fits> <index of dimension 0> ... <index of
// dimension C-1>" (check = operand_layout_check's code; the indices only when it is 0), then OK <lines>.  The judge is tests/test_operands_cpu.py (Python big integers).
#include <cinttypes>
#include <cstdio>
#include "../../lasso_amd/csrc/operand_layout.cuh"

int main(int argc, char** argv) {
  if (argc < 2) { fprintf(stderr, "usage: %s cases.txt\n", argv[0]); return 2; }
  FILE* f = fopen(argv[1], "r");
  if (!f) { perror(argv[1]); return 2; }
  lasso_operand_layout L; unsigned long long C, log_m; uint64_t x, y; size_t count = 0;
  while (fscanf(f, "%u %u %u %llu %llu %" SCNx64 " %" SCNx64, &L.operands, &L.chunk_bits, &L.msb_first, &C, &log_m, &x, &y) == 7) {
    const int bad = operand_layout_check(&L, (size_t)C, (size_t)log_m);
    printf("%d", bad);
    if (!bad) {
      printf(" %d %d", operand_fits(x, (size_t)C, L.chunk_bits) ? 1 : 0, operand_fits(y, (size_t)C, L.chunk_bits) ? 1 : 0);
      for (size_t dim = 0; dim < C; dim++) printf(" %" PRIu64, operand_index(L, x, y, (size_t)C, dim));
    }
    printf("\n");
    count++;
  }
  fclose(f);
  printf("OK %zu\n", count);
  return 0;
}
