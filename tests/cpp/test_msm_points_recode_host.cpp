// msmp_digit (lasso_amd/csrc/msm_points_recode.cuh) — the signed window recoding one lane of k_msmp_prepare runs per scalar — compiled for the host.
// argv[1]: a file of 64-hex-digit lines, one 256-bit little-endian integer each; argv[2..]: window widths c.  First line "C <the width the kernels are built with>",
// then per integer and width "<c> <digit 0> <digit 1> ...", then OK.  The judge is tests/test_msm_points_cpu.py (Python big integers).
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include "../../lasso_amd/csrc/msm_points_recode.cuh"

static int hexval(char c) { return c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10 : -1; }

int main(int argc, char** argv) {
  if (argc < 3) { fprintf(stderr, "usage: %s integers.hex c...\n", argv[0]); return 2; }
  FILE* f = fopen(argv[1], "r");
  if (!f) { perror(argv[1]); return 2; }
  printf("C %u\n", MSMP_C);
  char line[256]; size_t count = 0;
  while (fgets(line, sizeof line, f)) {
    if (strlen(line) < 64) continue;
    uint8_t b[32];
    for (int i = 0; i < 32; i++) { const int h = hexval(line[2 * i]), l = hexval(line[2 * i + 1]); if (h < 0 || l < 0) { fprintf(stderr, "bad hex\n"); return 2; } b[i] = (uint8_t)(h * 16 + l); }
    uint32_t s[8]; memcpy(s, b, 32);
    for (int a = 2; a < argc; a++) {
      const uint32_t c = (uint32_t)atoi(argv[a]);
      if (c < 2 || c > 16) { fprintf(stderr, "bad width\n"); return 2; }
      printf("%u", c);
      uint32_t carry = 0;
      for (uint32_t w = 0; w < MSMP_WINDOWS(c); w++) printf(" %d", msmp_digit(s, c, w, carry));
      if (carry) { fprintf(stderr, "carry out of the last window\n"); return 1; }
      printf("\n");
    }
    count++;
  }
  fclose(f);
  printf("OK %zu\n", count);
  return 0;
}
