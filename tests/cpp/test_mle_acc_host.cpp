// CPU driver of lasso_amd/csrc/mle_acc.cuh — the lazy sums of k_tables_mle — for tests/test_mle_cpu.py, which holds its output against Python big integers, once built
// plain and once with -fsanitize=undefined (a column that leaves its signed 64 bits is then a failure, not a wrong digit).
// stdin, any number of cases:   u32 <lo> <n>  then n lines  <t decimal> <e>        |        fr <lo> <n>  then n lines  <t> <e>
// (<lo>, <e>, field <t>: 64 hex digits, a 256-bit memory word, most significant digit first).  A case runs the kernel's own sequence — add, a carry pass every
// MLE_FOLD_EVERY (MLE_FR_FOLD_EVERY) terms, the last fold, the reduction — and prints two canonical integers as 64 hex digits each:
//   inner = A / 2^261 (mod p)   and   inner * lo / 2^261 (mod p),      A = sum t * e over the integers behind the words.
#include "../../lasso_amd/csrc/mle_acc.cuh"
#include <cstdio>
#include <cstring>
#include <string>

static bool parse_word(const char* s, fr_t& out) {
  if (strlen(s) != 64) return false;
  for (int w = 0; w < 8; w++) {
    uint32_t v = 0;
    for (int k = 0; k < 8; k++) {
      const char ch = s[64 - 8 * (w + 1) + k];
      const int d = ch >= '0' && ch <= '9' ? ch - '0' : ch >= 'a' && ch <= 'f' ? ch - 'a' + 10 : -1;
      if (d < 0) return false;
      v = v << 4 | (uint32_t)d;
    }
    out.v[w] = v;
  }
  return true;
}
static void print_canonical(const fr29& x) {
  const fr_t m = fr29_store(x);
  for (int w = 7; w >= 0; w--) printf("%08x", m.v[w]);
}

int main() {
  char form[8], a[80], b[80]; unsigned long n;
  while (scanf("%7s %79s %lu", form, a, &n) == 3) {
    const bool fr = strcmp(form, "fr") == 0;
    fr_t lo; if (!parse_word(a, lo)) { fprintf(stderr, "bad lo word\n"); return 2; }
    mle_acc acc = mle_acc_zero(); fr29_acc wide = fr29_acc_zero(); uint32_t cnt = 0;
    for (unsigned long i = 0; i < n; i++) {
      if (scanf("%79s %79s", a, b) != 2) { fprintf(stderr, "short case\n"); return 2; }
      fr_t e; if (!parse_word(b, e)) { fprintf(stderr, "bad e word\n"); return 2; }
      if (fr) {
        fr_t t; if (!parse_word(a, t)) { fprintf(stderr, "bad t word\n"); return 2; }
        mle_fr_acc_add(wide, fr29_unpack_u(t), fr29_unpack_u(e));
        if (++cnt == MLE_FR_FOLD_EVERY) { fr29_acc_carry(wide); cnt = 0; }
      } else {
        mle_acc_add_u32(acc, (uint32_t)strtoul(a, nullptr, 10), fr29_unpack_u(e));
        if (++cnt == MLE_FOLD_EVERY) { mle_acc_fold(acc); cnt = 0; }
      }
    }
    fr29 inner;
    if (fr) inner = mle_fr_acc_reduce(wide); else { mle_acc_fold(acc); inner = mle_acc_reduce(acc); }
    print_canonical(fr29_mul(inner, fr29_one_s())); printf(" ");
    print_canonical(fr29_mul(inner, fr29_unpack_u(lo))); printf("\n");
  }
  printf("periods %u %u\n", MLE_FOLD_EVERY, MLE_FR_FOLD_EVERY);
  return 0;
}
