// pt_decompress (lasso_amd/csrc/fe29.cuh, bn254_fe29.cuh with -DLASSO_BN254) — the function one lane of k_points_decompress runs — compiled for the host.
// argv[1]: a file of 64-hex-digit lines, one 32-byte encoding each.  Prints per line "<status> <affine: 128 hex digits> <canonical: 64 hex digits>", then OK.
// The judge is tests/test_wire_points_cpu.py (a big-integer decoder written from ark-ec's rules).
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include "../../lasso_amd/csrc/fe29.cuh"

static int hexval(char c) { return c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10 : -1; }

int main(int argc, char** argv) {
  if (argc < 2) { fprintf(stderr, "usage: %s encodings.hex\n", argv[0]); return 2; }
  FILE* f = fopen(argv[1], "r");
  if (!f) { perror(argv[1]); return 2; }
  char line[256]; size_t count = 0;
  while (fgets(line, sizeof line, f)) {
    if (strlen(line) < 64) continue;
    uint8_t b[32];
    for (int i = 0; i < 32; i++) { const int h = hexval(line[2 * i]), l = hexval(line[2 * i + 1]); if (h < 0 || l < 0) { fprintf(stderr, "bad hex\n"); return 2; } b[i] = (uint8_t)(h * 16 + l); }
    uint32_t in[8], aff[16], canon[8];
    memcpy(in, b, 32);
    const uint32_t st = pt_decompress(in, aff, canon);
    uint8_t a8[64], c8[32]; memcpy(a8, aff, 64); memcpy(c8, canon, 32);
    printf("%u ", st);
    for (int i = 0; i < 64; i++) printf("%02x", a8[i]);
    printf(" ");
    for (int i = 0; i < 32; i++) printf("%02x", c8[i]);
    printf("\n");
    count++;
  }
  fclose(f);
  printf("OK %zu\n", count);
  return 0;
}
