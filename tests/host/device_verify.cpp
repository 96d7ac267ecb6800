// TEST PROGRAM for verification on the device as the compiled host side reaches it (include/zkhip_backend.hpp: Hip::load_verification_key,
// Hip::verify_batch; include/zkhip.h: zkhip_vk_load_*, zkhip_verify_*_batch, zkhip_pairing_products), with the HOST verifier as the truth.
//
//   device_verify verify <curve id> <g16|gm17> <proving.key> <records> <inputs> <l>
//     records: n proof records (8 sz(Fq) + 3 bytes each) as the prove calls write them, inputs: n x l x 32 B little-endian.  Every record
//     becomes a Proof the way the host layer prints one (a flagged point as ark's zero (0, 1)); the key is the one at the head of the
//     proving key.  For every proof: the host `verify`; then ONE Hip::verify_batch over all of them and ONE zkhip_verify_*_batch over the
//     raw records: each verdict must be the host's.  Besides: a proof tagged with another curve is refused by name ("proof k"); the
//     key's bytes under another curve id are refused at load.  Prints "verdicts <0/1 per proof>".
//   device_verify pairs <curve id> <pairs per item> <file>
//     file: one pair per line, "P.x P.y Q.x.c0 Q.x.c1 Q.y.c0 Q.y.c1" in hex, items of <pairs per item> consecutive lines.  Per item the
//     host's pairing_product_is_one — which throws for a point outside its group: the device's verdict is then 0 — against
//     zkhip_pairing_products over all items in one call.  Prints "verdicts <0/1 per item>".
// Exit status 0 if everything agreed, 1 otherwise.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <sstream>

#include "../../include/zkhip_backend.hpp"

using namespace zokrates_hip;

static std::vector<uint8_t> slurp(const char* path) {
    std::ifstream f(path, std::ios::binary);
    return std::vector<uint8_t>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}
static int failures = 0;
static void expect(bool ok, const std::string& what) {
    if (ok) return;
    ++failures;
    fprintf(stderr, "device_verify: FAILED %s\n", what.c_str());
}
static std::string hex_be(const uint8_t* le, size_t n) {
    static const char* D = "0123456789abcdef";
    std::string s = "0x";
    for (size_t i = n; i-- > 0;) { s.push_back(D[le[i] >> 4]); s.push_back(D[le[i] & 15]); }
    return s;
}
static const char* curve_name(int id) { return id == 0 ? "bn128" : id == 1 ? "bls12_381" : "bls12_377"; }

static int run_verify(int curve, const std::string& scheme, const char* key_path, const char* rec_path, const char* in_path, size_t l) {
    const size_t fq = curve == 0 ? 32 : 48, rec = 8 * fq + 3;
    const std::vector<uint8_t> key = slurp(key_path), records = slurp(rec_path), inputs = slurp(in_path);
    const size_t n = records.size() / rec;
    expect(n * rec == records.size() && inputs.size() == n * l * 32, "the files' sizes");
    const Scheme sc = scheme == "gm17" ? Scheme::GM17 : Scheme::G16;
    const VerificationKey vk = VerificationKey::from_json(verification_key_json(sc, curve, key.data(), key.size()));
    std::vector<Proof> proofs;
    for (size_t i = 0; i < n; ++i) {
        std::vector<uint8_t> r(records.begin() + i * rec, records.begin() + (i + 1) * rec);
        std::vector<uint8_t> one(fq, 0);
        one[0] = 1;
        const size_t x_of[3] = {0, 2 * fq, 6 * fq}, len_of[3] = {2 * fq, 4 * fq, 2 * fq};
        for (int k = 0; k < 3; ++k)
            if (r[8 * fq + k]) {                                    // ark's zero(): (0, 1)
                memset(&r[x_of[k]], 0, len_of[k]);
                memcpy(&r[x_of[k] + len_of[k] / 2], one.data(), fq);
            }
        Proof p;
        p.scheme = scheme;
        p.curve = curve_name(curve);
        p.proof.a = {hex_be(&r[0], fq), hex_be(&r[fq], fq)};
        p.proof.b.x = {hex_be(&r[2 * fq], fq), hex_be(&r[3 * fq], fq)};
        p.proof.b.y = {hex_be(&r[4 * fq], fq), hex_be(&r[5 * fq], fq)};
        p.proof.c = {hex_be(&r[6 * fq], fq), hex_be(&r[7 * fq], fq)};
        for (size_t j = 0; j < l; ++j) p.inputs.push_back(hex_be(&inputs[(i * l + j) * 32], 32));
        proofs.push_back(p);
    }
    std::vector<bool> host;
    for (size_t i = 0; i < n; ++i) host.push_back(verify(vk, proofs[i]));
    Hip hip(0);
    const DeviceVerificationKey dvk = hip.load_verification_key(vk);
    expect(dvk.inputs() == l && dvk.scheme() == scheme && dvk.curve() == curve_name(curve), "the loaded key's shape");
    const std::vector<bool> dev = hip.verify_batch(dvk, proofs);
    expect(dev.size() == n, "one verdict per proof");
    for (size_t i = 0; i < n && i < dev.size(); ++i) expect(dev[i] == host[i], "Hip::verify_batch against verify, proof " + std::to_string(i));
    expect(hip.verify_batch(dvk, {}).empty(), "an empty batch");
    // the raw records (flags as the prover set them) through the C ABI, a context of the program's own
    zkhip_ctx* ctx = nullptr;
    expect(zkhip_ctx_create(0, &ctx) == ZKHIP_OK, "zkhip_ctx_create");
    zkhip_vk* raw_vk = nullptr;
    const auto load = sc == Scheme::GM17 ? zkhip_vk_load_gm17 : zkhip_vk_load_g16;
    expect(load(ctx, curve, key.data(), key.size(), &raw_vk) == ZKHIP_OK, "zkhip_vk_load");
    std::vector<uint8_t> ok(n, 0xff);
    const auto call = sc == Scheme::GM17 ? zkhip_verify_gm17_batch : zkhip_verify_g16_batch;
    expect(call(ctx, raw_vk, n, records.data(), l ? inputs.data() : nullptr, ok.data()) == ZKHIP_OK, std::string("zkhip_verify_*_batch: ") + zkhip_last_error(ctx));
    for (size_t i = 0; i < n; ++i) expect(ok[i] == (host[i] ? 1 : 0), "zkhip_verify_*_batch against verify, proof " + std::to_string(i));
    // a curve mismatch: the key's bytes under another curve id, a proof tagged with another curve
    zkhip_vk* wrong = nullptr;
    const int32_t rc = load(ctx, curve == 0 ? 1 : 0, key.data(), key.size(), &wrong);
    expect(rc == ZKHIP_ERR_PARSE && wrong == nullptr, "a key loaded under another curve id is refused, rc " + std::to_string(rc));
    if (n >= 2) {
        std::vector<Proof> tagged(proofs.begin(), proofs.begin() + 2);
        tagged[1].curve = curve == 0 ? "bls12_381" : "bn128";
        try {
            hip.verify_batch(dvk, tagged);
            expect(false, "a proof of another curve is refused");
        } catch (const Error& e) {
            expect(e.code == ZKHIP_ERR_BAD_ARG && std::string(e.what()).find("proof 1: Expected the curve") == 0, std::string("the refusal names the proof: ") + e.what());
        }
        bool threw = false;
        try { verify(vk, tagged[1]); } catch (const Error&) { threw = true; }
        expect(threw, "the host verifier refuses it too");
        std::vector<Proof> extra(proofs.begin(), proofs.begin() + 2);
        extra[1].inputs.push_back(hex_be(inputs.data(), 0) + "01");
        try {
            hip.verify_batch(dvk, extra);
            expect(false, "an input too many is refused");
        } catch (const Error& e) {
            expect(e.code == ZKHIP_ERR_BAD_ARG && std::string(e.what()).find("proof 1: ") == 0, std::string("the refusal names the proof: ") + e.what());
        }
    }
    zkhip_vk_free(raw_vk);
    zkhip_ctx_free(ctx);
    std::string line;
    for (size_t i = 0; i < n; ++i) line.push_back(host[i] ? '1' : '0');
    printf("verdicts %s\n", line.c_str());
    return failures ? 1 : 0;
}

static int run_pairs(int curve, size_t per_item, const char* path) {
    const size_t fq = curve == 0 ? 32 : 48;
    std::ifstream f(path);
    std::vector<std::pair<G1Affine, G2Affine>> pairs;
    std::string ln;
    while (std::getline(f, ln)) {
        std::istringstream is(ln);
        std::string t[6];
        for (auto& s : t) is >> s;
        if (t[5].empty()) continue;
        pairs.push_back({G1Affine{t[0], t[1]}, G2Affine{{t[2], t[3]}, {t[4], t[5]}}});
    }
    const size_t n = pairs.size() / per_item;
    expect(n * per_item == pairs.size() && n > 0, "whole items");
    std::vector<uint8_t> g1, g2;
    for (const auto& pr : pairs) {
        detail::g1_le(pr.first, fq, g1); g1.push_back(0);
        detail::g2_le(pr.second, fq, g2); g2.push_back(0);
    }
    zkhip_ctx* ctx = nullptr;
    expect(zkhip_ctx_create(0, &ctx) == ZKHIP_OK, "zkhip_ctx_create");
    std::vector<uint8_t> ok(n, 0xff);
    expect(zkhip_pairing_products(ctx, curve, n, (uint32_t)per_item, g1.data(), g2.data(), ok.data()) == ZKHIP_OK, std::string("zkhip_pairing_products: ") + zkhip_last_error(ctx));
    std::string line;
    for (size_t i = 0; i < n; ++i) {
        bool host = false;
        try {
            host = pairing_product_is_one(curve_name(curve), std::vector<std::pair<G1Affine, G2Affine>>(pairs.begin() + i * per_item, pairs.begin() + (i + 1) * per_item));
        } catch (const Error&) {}                                   // a point outside its group: the device answers 0
        expect(ok[i] == (host ? 1 : 0), "zkhip_pairing_products against pairing_product_is_one, item " + std::to_string(i));
        line.push_back(host ? '1' : '0');
    }
    zkhip_ctx_free(ctx);
    printf("verdicts %s\n", line.c_str());
    return failures ? 1 : 0;
}

int main(int argc, char** argv) {
    try {
        if (argc == 8 && std::string(argv[1]) == "verify") return run_verify(atoi(argv[2]), argv[3], argv[4], argv[5], argv[6], (size_t)atol(argv[7]));
        if (argc == 5 && std::string(argv[1]) == "pairs") return run_pairs(atoi(argv[2]), (size_t)atol(argv[3]), argv[4]);
        return 2;
    } catch (const std::exception& e) {
        fprintf(stderr, "device_verify: %s\n", e.what());
        return 1;
    }
}
