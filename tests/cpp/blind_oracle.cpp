// Test-only harness: the hiding form of the dense polynomial commitment by the ORACLE (oracle/lasso_oracle.hpp, included and not edited), linked beside the host prover so
// that one library answers both sides of tests/test_blind_cpu.py.  Rows by batch_commit(row, n, blind, gens_n); PolyEvalProof::prove with blinds (dense_mlpoly.rs:302-359)
// restated over the oracle's dot_product_log_prove(.., blind_x, .., blind_y, &Cx, &Cy); PolyEvalProof::verify (:361-386) over its dot_product_log_verify.
// Scalars cross the boundary as 4 x u64 memory words (Montgomery form), points as 32 wire bytes.
#include <cstring>
#include <string>
#include <vector>
#include "../../oracle/lasso_oracle.hpp"

using namespace orc;

namespace {
std::vector<Fr> scalars(const u64* w, size_t n) { std::vector<Fr> v; v.reserve(n); for (size_t i = 0; i < n; i++) v.push_back(Fr::from_raw(w + 4 * i)); return v; }
void put(const Fr& x, u64* w) { memcpy(w, x.v, 32); }
}  // namespace

extern "C" {
// DensePolynomial::commit(gens, Some(tape)) then PolyEvalProof::prove(poly, blinds, r, Zr, blind_Zr, gens, transcript, tape) on ONE tape RandomTape::new(tape_label) and a
// transcript Transcript::new(t_label).  with_blinds = 0: the opening passes None for the row blinds (the commitment is blinded all the same); blind_Zr may be NULL (None).
// Out: blinds (L scalars), rows (L x 32 B), Zr, C_Zr' (32 B), the serialized DotProductProofLog.  Returns 0, -2 when cap is too small, -1 on an oracle assertion.
int blind_orc_commit_open(const char* gens_label, size_t num_vars, const u64* Z, const u64* r, int with_blinds, const u64* blind_Zr, const char* t_label, const char* tape_label,
                          u64* blinds_out, uint8_t* rows_out, u64* Zr_out, uint8_t* C_Zr_out, uint8_t* proof_out, size_t cap, size_t* len) {
  try {
    const PolyCommitmentGens gens = PolyCommitmentGens::create(num_vars, gens_label);
    const DensePolynomial poly(scalars(Z, (size_t)1 << num_vars));
    const auto lens = EqPolynomial::compute_factored_lens(num_vars);
    const size_t L_size = pow2(lens.first), R_size = pow2(lens.second);
    RandomTape tape(tape_label);
    const std::vector<Fr> blinds = tape.random_vector("poly_blinds", L_size);   // dense_mlpoly.rs:166-170
    for (size_t i = 0; i < L_size; i++) {
      put(blinds[i], blinds_out + 4 * i);
      batch_commit(&poly.Z[R_size * i], R_size, blinds[i], gens.gens.gens_n).compress(rows_out + 32 * i);   // commit_inner :110-150
    }
    MerlinTranscript t(t_label);
    t.append_protocol_name("polynomial evaluation proof");
    const auto LR = EqPolynomial(scalars(r, num_vars)).compute_factored_evals();
    const std::vector<Fr> LZ = poly.bound(LR.first);
    Fr LZ_blind = Fr::zero();
    if (with_blinds) for (size_t i = 0; i < L_size; i++) LZ_blind += LR.first[i] * blinds[i];   // :330-333
    const Fr Zr = compute_dotproduct(LZ.data(), LR.second.data(), R_size);
    Point Cx, Cy;
    const DotProductProofLog p = dot_product_log_prove(gens.gens, t, tape, LZ, LZ_blind, LR.second, Zr, blind_Zr ? Fr::from_raw(blind_Zr) : Fr::zero(), &Cx, &Cy);
    put(Zr, Zr_out);
    Cy.compress(C_Zr_out);
    ByteWriter w; w.dpl(p);
    *len = w.b.size();
    if (w.b.size() > cap) return -2;
    memcpy(proof_out, w.b.data(), w.b.size());
    return 0;
  } catch (...) { return -1; }
}
// PolyEvalProof::verify(gens, transcript, r, C_Zr, comm) on Transcript::new(t_label): 1 = Ok, 0 = Err, -1 = bytes that do not deserialize
int blind_orc_verify(const char* gens_label, size_t num_vars, const u64* r, const uint8_t* C_Zr, const char* t_label, const uint8_t* proof, size_t proof_len, const uint8_t* rows, size_t n_rows) {
  try {
    const PolyCommitmentGens gens = PolyCommitmentGens::create(num_vars, gens_label);
    ByteReader pr(proof, proof_len);
    const DotProductProofLog p = pr.dpl();
    if (!pr.ok || pr.pos != proof_len) return -1;
    Point Cy; if (!curve_decompress(C_Zr, Cy)) return -1;
    PolyCommitment comm(n_rows);
    for (size_t i = 0; i < n_rows; i++) if (!curve_decompress(rows + 32 * i, comm[i])) return -1;
    MerlinTranscript t(t_label);
    t.append_protocol_name("polynomial evaluation proof");
    const auto LR = EqPolynomial(scalars(r, num_vars)).compute_factored_evals();
    if (LR.first.size() != n_rows) return -1;
    const Point C_LZ = msm(comm, LR.first);
    return dot_product_log_verify(p, LR.second.size(), gens.gens, t, LR.second, C_LZ, Cy) ? 1 : 0;
  } catch (...) { return -1; }
}
}
