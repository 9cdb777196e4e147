// The per-item-key overloads of include/bbs_sign_amd.hpp meet their issuers one call after another: proof_verify_batch with one
// PublicKey per item three times, with 2, then 3, then 5 distinct issuers.  Every result is what the single-key function
// gives and what the items were made to be (valid, forged, presented under another issuer's key), and the context's key set
// grows 2 -> 3 -> 5: the wrapper appends the keys it has not seen, it does not register the union again.  Built by
// tests/test_keyreg_hosttwin.py / tests/test_keyreg_gpu.py with g++ -std=c++17.
#include <cstdio>
#include <cstdlib>

#include "bbs_sign_amd.hpp"

using namespace bbs_plus;

#define CHECK(cond) do { if (!(cond)) { std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); std::exit(1); } } while (0)

static Bytes B(const std::string& s) { return Bytes(s.begin(), s.end()); }

static void run(Curve c) {
    const size_t K = 5, L = 3;
    std::vector<SecretKey> sks;
    std::vector<PublicKey> issuers;
    for (size_t k = 0; k < K; k++) {
        sks.push_back(SecretKey::key_gen(c, Bytes(32, (uint8_t)(31 + k)), {}, B("BBS-SIG-KEYGEN-SALT-")).unwrap());
        issuers.push_back(sks.back().sk_to_pk());
    }
    const size_t rounds[3] = {2, 3, 5};
    const std::vector<size_t> d = {0, 2};
    size_t item = 0;
    for (int r = 0; r < 3; r++) {
        const size_t k_now = rounds[r], n = 2 * k_now + 1;
        std::vector<PublicKey> pks;
        std::vector<Proof> proofs;
        std::vector<Bytes> headers, phs;
        std::vector<std::vector<Bytes>> dmsgs;
        std::vector<std::vector<size_t>> didx;
        std::vector<bool> truth;
        for (size_t i = 0; i < n; i++, item++) {
            const size_t owner = i % k_now;
            std::vector<Bytes> m;
            for (size_t j = 0; j < L; j++) m.push_back(B("round" + std::to_string(r) + "-item" + std::to_string(item) + "-msg" + std::to_string(j)));
            const Bytes h = B("header" + std::to_string(item % 3)), ph = B("ph" + std::to_string(item));
            const Signature sig = sks[owner].sign(m, h).unwrap();
            proofs.push_back(proof_gen(issuers[owner], sig, h, ph, m, d).unwrap());
            const bool forged = i == 1, other_key = i == 2;
            dmsgs.push_back({forged ? B("forged") : m[0], m[2]});
            didx.push_back(d);
            headers.push_back(h);
            phs.push_back(ph);
            pks.push_back(issuers[other_key ? (owner + 1) % k_now : owner]);
            truth.push_back(!forged && !other_key);
        }
        const auto got = proof_verify_batch(pks, proofs, headers, phs, dmsgs, didx, L);
        CHECK(got.size() == n);
        for (size_t i = 0; i < n; i++) {
            const auto want = proof_verify(pks[i], proofs[i], headers[i], phs[i], dmsgs[i], didx[i]);
            CHECK(got[i].error == want.error && got[i].value == want.value);
            CHECK(got[i].unwrap() == truth[i]);
        }
        CHECK(bbs_ctx_public_key_count(detail::keyed_context(c, L)->ctx.get()) == k_now);
    }
}

int main() {
    run(Curve::Bls12_381);
    run(Curve::Bn254);
    std::printf("all checks passed\n");
    return 0;
}
