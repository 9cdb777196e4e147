// SecretKey::key_gen_batch / sk_to_pk_batch of include/bbs_sign_amd.hpp: a batch of 70 keys per curve against a loop over
// SecretKey::key_gen, the two error variants inside a batch, and key material that is zero after the call.
// The 70 public keys are compared with bbs_ctx_set_secret_key + bbs_ctx_get_public_key on ONE context -- the two calls
// SecretKey::sk_to_pk() is made of -- and sk_to_pk() itself is called for three of them: it keeps a context with generator
// tables per secret key, which seventy keys per curve would multiply on the device.
// Built by tests/test_keygen_hosttwin.py / tests/test_keygen_gpu.py with g++ -std=c++17.
#include <cstdio>
#include <cstdlib>

#include "bbs_sign_amd.hpp"

using namespace bbs_plus;

#define CHECK(cond) do { if (!(cond)) { std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); std::exit(1); } } while (0)

static Bytes B(const std::string& s) { return Bytes(s.begin(), s.end()); }

static void run(Curve c) {
    const size_t n = 70, SHORT_AT = 17, LONG_AT = 63;
    const Bytes dst = B("BBS-SIG-KEYGEN-SALT-");
    std::vector<Bytes> kms, kis;
    for (size_t k = 0; k < n; k++) {
        Bytes km(32 + k % 9), ki(k % 5);
        for (size_t i = 0; i < km.size(); i++) km[i] = (uint8_t)(1 + 3 * k + 7 * i);
        for (size_t i = 0; i < ki.size(); i++) ki[i] = (uint8_t)(k + i);
        kms.push_back(km);
        kis.push_back(ki);
    }
    kms[SHORT_AT].resize(31);                                  // InvalidKeyMaterialLength
    kis[LONG_AT].assign(65536, 0x5a);                          // InvalidKeyInfoLength
    // the loop a caller had before
    std::vector<Result<SecretKey>> want;
    for (size_t k = 0; k < n; k++) want.push_back(SecretKey::key_gen(c, kms[k], kis[k], dst));
    std::vector<Bytes> material = kms;
    const auto got = SecretKey::key_gen_batch(c, material, kis, dst);
    CHECK(got.size() == n);
    CHECK(got[SHORT_AT].error == BBS_ST_INVALID_KEY_MATERIAL_LENGTH && want[SHORT_AT].error == BBS_ST_INVALID_KEY_MATERIAL_LENGTH);
    CHECK(got[LONG_AT].error == BBS_ST_INVALID_KEY_INFO_LENGTH && want[LONG_AT].error == BBS_ST_INVALID_KEY_INFO_LENGTH);
    // key material is cleared in place, every item's
    for (size_t k = 0; k < n; k++) {
        CHECK(material[k].size() == kms[k].size());
        for (uint8_t b : material[k]) CHECK(b == 0);
    }
    bbs_ctx* scratch = nullptr;
    CHECK(bbs_ctx_create((int)c, 0, &scratch) == BBS_OK);
    const size_t fpb = bbs_fp_bytes((int)c);
    std::vector<SecretKey> sks;
    for (size_t k = 0; k < n; k++) {
        CHECK(got[k].error == want[k].error);
        if (got[k].is_err()) continue;
        const auto& kp = got[k].value;
        CHECK(kp.first.curve == c && kp.second.curve == c && kp.first.sk == want[k].value.sk);
        Bytes pk(4 * fpb);
        int inf = 1;
        CHECK(bbs_ctx_set_secret_key(scratch, kp.first.sk.data()) == BBS_OK);
        CHECK(bbs_ctx_get_public_key(scratch, pk.data(), &inf) == BBS_OK);
        CHECK(inf == 0 && !kp.second.identity && kp.second.pk == pk);
        if (k == 0 || k == 64 || k == n - 1) {
            const PublicKey one = kp.first.sk_to_pk();
            CHECK(one.pk == kp.second.pk && one.identity == kp.second.identity);
        }
        sks.push_back(kp.first);
    }
    bbs_ctx_destroy(scratch);
    CHECK(sks.size() == n - 2);
    // sk_to_pk_batch: the same keys again, and the identity key for sk = 0
    SecretKey zero;
    zero.curve = c;
    sks.push_back(zero);
    const auto pks = SecretKey::sk_to_pk_batch(sks);
    CHECK(pks.size() == sks.size());
    size_t j = 0;
    for (size_t k = 0; k < n; k++) {
        if (got[k].is_err()) continue;
        CHECK(pks[j].pk == got[k].value.second.pk && !pks[j].identity && pks[j].curve == c);
        j++;
    }
    CHECK(pks[j].identity && pks[j].pk == Bytes(4 * fpb, 0));
    // a key pair of the batch signs and verifies through the existing functions
    const auto& kp = got[5].value;
    const std::vector<Bytes> msgs = {B("one message")};
    const Signature sig = kp.first.sign(msgs, B("header")).unwrap();
    CHECK(kp.second.verify(sig, B("header"), msgs).unwrap());
    // what key_gen throws on, key_gen_batch throws on: a key_dst of more than 255 bytes
    std::vector<Bytes> two = {kms[0], kms[1]};
    bool thrown = false;
    try { (void)SecretKey::key_gen_batch(c, two, {kis[0], kis[1]}, Bytes(256, 1)); } catch (const std::runtime_error&) { thrown = true; }
    CHECK(thrown);
    CHECK(SecretKey::sk_to_pk_batch({}).empty());
}

int main() {
    run(Curve::Bls12_381);
    run(Curve::Bn254);
    std::printf("all checks passed\n");
    return 0;
}
