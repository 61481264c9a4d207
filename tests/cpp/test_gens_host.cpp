// pt_from_candidate (lasso_amd/csrc/fe29.cuh, bn254_fe29.cuh with -DLASSO_BN254) — the function one lane of k_points_from_candidates runs — compiled for the host, next to
// the host prover's own point_from_candidate (lasso_amd/host/prover.hpp).
// argv[1]: a file of lines "<64 hex digits: the 32 bytes of the limbs> <0|1: greatest>".  argv[2]: how many candidates of the label argv[3] to draw first.
// The two functions are compared here, status for status and limb for limb, on every candidate (a mismatch ends the program with status 1); per line of the file
// "<status> <affine: 128 hex digits>" is printed, per stream candidate "S <limbs: 64 hex digits> <greatest>", then OK.  The judge of the printed values is
// tests/test_gens_device_cpu.py (a big-integer statement written from ark-ec's rules, and an independent statement of the stream).
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include "../../lasso_amd/host/prover.hpp"
#include "../../lasso_amd/csrc/fe29.cuh"

using namespace lasso;

static int hexval(char c) { return c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10 : -1; }

// both implementations on one candidate; false = they differ
static bool both(const uint64_t* limbs, bool greatest, uint32_t& st, uint8_t a8[64]) {
  uint32_t in[8], aff[16];
  memcpy(in, limbs, 32);
  st = pt_from_candidate(in, greatest, aff);
  memcpy(a8, aff, 64);
  Pt p; lasso_affine h; memset(&h, 0, sizeof h);
  const uint32_t hs = point_from_candidate(limbs, greatest, p);
  if (hs == LASSO_CAND_OK) normalize_points(&p, 1, &h);
  if (hs != st || memcmp(&h, a8, 64) != 0) {
    fprintf(stderr, "mismatch: device form status %u, host status %u, limbs %016llx %016llx %016llx %016llx greatest %d\n", st, hs, (unsigned long long)limbs[0], (unsigned long long)limbs[1],
            (unsigned long long)limbs[2], (unsigned long long)limbs[3], (int)greatest);
    return false;
  }
  return true;
}

int main(int argc, char** argv) {
  if (argc < 4) { fprintf(stderr, "usage: %s candidates.txt stream_count label\n", argv[0]); return 2; }
  FILE* f = fopen(argv[1], "r");
  if (!f) { perror(argv[1]); return 2; }
  char line[256]; size_t count = 0;
  while (fgets(line, sizeof line, f)) {
    if (strlen(line) < 66) continue;
    uint8_t b[32];
    for (int i = 0; i < 32; i++) { const int h = hexval(line[2 * i]), l = hexval(line[2 * i + 1]); if (h < 0 || l < 0) { fprintf(stderr, "bad hex\n"); return 2; } b[i] = (uint8_t)(h * 16 + l); }
    uint64_t limbs[4]; memcpy(limbs, b, 32);
    uint32_t st; uint8_t a8[64];
    if (!both(limbs, line[65] == '1', st, a8)) return 1;
    printf("%u ", st);
    for (int i = 0; i < 64; i++) printf("%02x", a8[i]);
    printf("\n");
    count++;
  }
  fclose(f);
  // the first candidates of the label's stream, drawn as GenStream draws them
  const size_t want = (size_t)atoll(argv[2]);
  Shake256 sh; sh.update(argv[3], strlen(argv[3]));
  uint8_t buf[32]; compress_generator(buf); sh.update(buf, 32);
  uint8_t seed[32]; sh.read(seed, 32);
  ChaChaRng rng(seed, 20);
  size_t ok = 0;
  for (size_t i = 0; i < want; i++) {
    const Candidate c = draw_candidate(rng);
    uint32_t st; uint8_t a8[64];
    if (!both(c.limbs, c.greatest, st, a8)) return 1;
    ok += st == LASSO_CAND_OK;
    uint8_t l8[32]; memcpy(l8, c.limbs, 32);
    printf("S ");
    for (int k = 0; k < 32; k++) printf("%02x", l8[k]);
    printf(" %d %u ", c.greatest ? 1 : 0, st);
    for (int k = 0; k < 64; k++) printf("%02x", a8[k]);
    printf("\n");
  }
  printf("OK %zu %zu %zu\n", count, want, ok);
  return 0;
}
