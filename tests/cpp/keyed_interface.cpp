// The per-item-key overloads of include/bbs_sign_amd.hpp (bbs_plus::proof_verify_batch / verify_batch with one PublicKey
// per item) against the single-key functions, item by item: three issuers, items presented under their own key, under
// another issuer's key, forged, and with different message counts.  Built by tests/test_keyed_cpp.py with g++ -std=c++17
// against the product library (GPU) or the CPU-side test build of the same stage code.
#include <cstdio>
#include <cstdlib>

#include "bbs_sign_amd.hpp"

using namespace bbs_plus;

#define CHECK(cond) do { if (!(cond)) { std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); std::exit(1); } } while (0)

static Bytes B(const std::string& s) { return Bytes(s.begin(), s.end()); }

static void run(Curve c) {
    std::vector<SecretKey> sks;
    std::vector<PublicKey> issuers;
    for (int k = 0; k < 3; k++) {
        sks.push_back(SecretKey::key_gen(c, Bytes(32, (uint8_t)(11 + k)), {}, B("BBS-SIG-KEYGEN-SALT-")).unwrap());
        issuers.push_back(sks.back().sk_to_pk());
    }
    const size_t n = 12;
    std::vector<PublicKey> pks;
    std::vector<Signature> sigs;
    std::vector<Proof> proofs;
    std::vector<Bytes> headers, phs;
    std::vector<std::vector<Bytes>> msgs, dmsgs;
    std::vector<std::vector<size_t>> didx;
    for (size_t i = 0; i < n; i++) {
        const size_t owner = i % 3;
        const size_t L = (i % 4 == 3) ? 2 : 3;                         // two message counts (verify groups by count)
        std::vector<Bytes> m;
        for (size_t j = 0; j < L; j++) m.push_back(B("item" + std::to_string(i) + "-msg" + std::to_string(j)));
        const Bytes h = B("header" + std::to_string(i % 2));
        sigs.push_back(sks[owner].sign(m, h).unwrap());
        msgs.push_back(m);
        headers.push_back(h);
        phs.push_back(B("ph" + std::to_string(i)));
        size_t presented = owner;
        if (i == 4) presented = (owner + 1) % 3;                       // another issuer's key
        pks.push_back(issuers[presented]);
    }
    msgs[7][0] = B("forged");                                          // a forged message
    // proof_verify needs one message count per call: the items with 3 messages
    std::vector<size_t> pv_items;
    for (size_t i = 0; i < n; i++) if (msgs[i].size() == 3) pv_items.push_back(i);
    std::vector<PublicKey> ppks;
    for (size_t i : pv_items) {
        const std::vector<size_t> d = {0, 2};
        Proof p = proof_gen(issuers[i % 3], sigs[i], headers[i], phs[i], msgs[i], d).unwrap();
        proofs.push_back(p);
        dmsgs.push_back({msgs[i][0], msgs[i][2]});
        didx.push_back(d);
        ppks.push_back(pks[i]);
    }
    std::vector<Bytes> ph_sel, h_sel;
    for (size_t i : pv_items) { ph_sel.push_back(phs[i]); h_sel.push_back(headers[i]); }
    const auto pr = proof_verify_batch(ppks, proofs, h_sel, ph_sel, dmsgs, didx, 3);
    CHECK(pr.size() == pv_items.size());
    size_t ones = 0;
    for (size_t t = 0; t < pv_items.size(); t++) {
        const auto want = proof_verify(ppks[t], proofs[t], h_sel[t], ph_sel[t], dmsgs[t], didx[t]);
        CHECK(pr[t].error == want.error && pr[t].value == want.value);
        // the single-key batch form agrees too
        const auto one = proof_verify_batch(ppks[t], {proofs[t]}, {h_sel[t]}, {ph_sel[t]}, {dmsgs[t]}, {didx[t]}, 3);
        CHECK(one[0].value == pr[t].value);
        ones += pr[t].value ? 1 : 0;
    }
    CHECK(ones > 0 && ones < pv_items.size());
    const auto vr = verify_batch(pks, sigs, headers, msgs);
    CHECK(vr.size() == n);
    for (size_t i = 0; i < n; i++) {
        const auto want = pks[i].verify(sigs[i], headers[i], msgs[i]);
        CHECK(vr[i].error == want.error && vr[i].value == want.value);
    }
    CHECK(!vr[4].unwrap() && !vr[7].unwrap() && vr[0].unwrap() && vr[3].unwrap());
    // a key that bbs_ctx_set_public_key refuses throws, as in the single-key functions
    PublicKey bad = issuers[0];
    bad.pk[0] ^= 1;
    bool threw = false;
    try { verify_batch({bad}, {sigs[0]}, {headers[0]}, {msgs[0]}); } catch (const std::exception&) { threw = true; }
    CHECK(threw);
    // and the context keeps serving afterwards
    const auto again = verify_batch(pks, sigs, headers, msgs);
    for (size_t i = 0; i < n; i++) CHECK(again[i].value == vr[i].value);
}

int main() {
    run(Curve::Bls12_381);
    run(Curve::Bn254);
    std::printf("all checks passed\n");
    return 0;
}
