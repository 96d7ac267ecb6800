// backend.cpp — zkhip_backend.hpp: the compiled host side of the `hip` backend (plain C++17 over the C ABI of zkhip.h; no
// HIP, no internal headers).  What it restates and where the reference does it:
//   * generate_proof        /root/reference/zokrates_ark/src/groth16.rs:20-53, gm17.rs:43-78 (inputs, key, prove, points)
//   * the blinding scalars  ark_groth16::create_random_proof draws `Fr::rand(rng)` twice (r, s), ark_gm17 three times
//                           (d1, d2, r), first thing, from the caller's RNG
//   * get_rng_from_entropy  /root/reference/zokrates_proof_systems/src/rng.rs:5-20 (Blake2b-512, first 32 bytes -> StdRng)
//   * StdRng                rand 0.8.5 = rand_chacha 0.3.1 ChaCha12Rng ([UPSTREAM]; known answers in tests/)
//   * Fr::rand              ark-ff 0.3.0 `impl Distribution<Fp256<P>> for Standard` ([UPSTREAM])
//   * proof points -> hex   parse_g1 / parse_g2 / parse_fr, /root/reference/zokrates_ark/src/lib.rs:150-226
//   * proof.json            TaggedProof + serde_json::to_string_pretty, /root/reference/zokrates_proof_systems/src/tagged.rs:14-37
#include "../../../include/zkhip_backend.hpp"

#include <chrono>
#include <cstdio>
#include <cstring>

namespace zokrates_hip {

// ------------------------------------------------------------------ BLAKE2b-512 (RFC 7693), unkeyed
namespace {
const uint64_t B2_IV[8] = {0x6a09e667f3bcc908ull, 0xbb67ae8584caa73bull, 0x3c6ef372fe94f82bull, 0xa54ff53a5f1d36f1ull,
                           0x510e527fade682d1ull, 0x9b05688c2b3e6c1full, 0x1f83d9abfb41bd6bull, 0x5be0cd19137e2179ull};
const uint8_t B2_SIGMA[12][16] = {
    {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15}, {14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3},
    {11, 8, 12, 0, 5, 2, 15, 13, 10, 14, 3, 6, 7, 1, 9, 4}, {7, 9, 3, 1, 13, 12, 11, 14, 2, 6, 5, 10, 4, 0, 15, 8},
    {9, 0, 5, 7, 2, 4, 10, 15, 14, 1, 11, 12, 6, 8, 3, 13}, {2, 12, 6, 10, 0, 11, 8, 3, 4, 13, 7, 5, 15, 14, 1, 9},
    {12, 5, 1, 15, 14, 13, 4, 10, 0, 7, 6, 3, 9, 2, 8, 11}, {13, 11, 7, 14, 12, 1, 3, 9, 5, 0, 15, 4, 8, 6, 2, 10},
    {6, 15, 14, 9, 11, 3, 0, 8, 12, 2, 13, 7, 1, 4, 10, 5}, {10, 2, 8, 4, 7, 6, 1, 5, 15, 11, 9, 14, 3, 12, 13, 0},
    {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15}, {14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3}};
inline uint64_t rotr64(uint64_t x, int n) { return (x >> n) | (x << (64 - n)); }
void b2_compress(uint64_t h[8], const uint8_t block[128], uint64_t t, bool last) {
    uint64_t m[16], v[16];
    for (int i = 0; i < 16; ++i) memcpy(&m[i], block + 8 * i, 8);   // little-endian host
    for (int i = 0; i < 8; ++i) { v[i] = h[i]; v[i + 8] = B2_IV[i]; }
    v[12] ^= t;                                                      // (messages here are far below 2^64 bytes: t1 = 0)
    if (last) v[14] = ~v[14];
    auto G = [&](int a, int b, int c, int d, uint64_t x, uint64_t y) {
        v[a] = v[a] + v[b] + x; v[d] = rotr64(v[d] ^ v[a], 32);
        v[c] = v[c] + v[d];     v[b] = rotr64(v[b] ^ v[c], 24);
        v[a] = v[a] + v[b] + y; v[d] = rotr64(v[d] ^ v[a], 16);
        v[c] = v[c] + v[d];     v[b] = rotr64(v[b] ^ v[c], 63);
    };
    for (int r = 0; r < 12; ++r) {
        const uint8_t* s = B2_SIGMA[r];
        G(0, 4, 8, 12, m[s[0]], m[s[1]]);   G(1, 5, 9, 13, m[s[2]], m[s[3]]);
        G(2, 6, 10, 14, m[s[4]], m[s[5]]);  G(3, 7, 11, 15, m[s[6]], m[s[7]]);
        G(0, 5, 10, 15, m[s[8]], m[s[9]]);  G(1, 6, 11, 12, m[s[10]], m[s[11]]);
        G(2, 7, 8, 13, m[s[12]], m[s[13]]); G(3, 4, 9, 14, m[s[14]], m[s[15]]);
    }
    for (int i = 0; i < 8; ++i) h[i] ^= v[i] ^ v[i + 8];
}
}  // namespace

std::array<uint8_t, 64> blake2b_512(const uint8_t* data, size_t len) {
    uint64_t h[8];
    for (int i = 0; i < 8; ++i) h[i] = B2_IV[i];
    h[0] ^= 0x01010040ull;                                           // digest length 64, no key, fanout = depth = 1
    uint8_t block[128];
    size_t off = 0;
    while (len - off > 128) {                                        // every block but the last
        b2_compress(h, data + off, (uint64_t)off + 128, false);
        off += 128;
    }
    memset(block, 0, 128);
    if (len > off) memcpy(block, data + off, len - off);
    b2_compress(h, block, (uint64_t)len, true);
    std::array<uint8_t, 64> out;
    memcpy(out.data(), h, 64);
    return out;
}

// ------------------------------------------------------------------ StdRng = ChaCha12
namespace {
inline uint32_t rotl32(uint32_t x, int n) { return (x << n) | (x >> (32 - n)); }
void chacha_block(const uint32_t key[8], uint64_t counter, uint64_t stream, int rounds, uint32_t out[16]) {
    const uint32_t init[16] = {0x61707865u, 0x3320646eu, 0x79622d32u, 0x6b206574u, key[0], key[1], key[2], key[3], key[4], key[5], key[6], key[7],
                               (uint32_t)counter, (uint32_t)(counter >> 32), (uint32_t)stream, (uint32_t)(stream >> 32)};
    uint32_t x[16];
    memcpy(x, init, sizeof(x));
    auto qr = [&](int a, int b, int c, int d) {
        x[a] += x[b]; x[d] = rotl32(x[d] ^ x[a], 16);
        x[c] += x[d]; x[b] = rotl32(x[b] ^ x[c], 12);
        x[a] += x[b]; x[d] = rotl32(x[d] ^ x[a], 8);
        x[c] += x[d]; x[b] = rotl32(x[b] ^ x[c], 7);
    };
    for (int r = 0; r < rounds / 2; ++r) {
        qr(0, 4, 8, 12); qr(1, 5, 9, 13); qr(2, 6, 10, 14); qr(3, 7, 11, 15);
        qr(0, 5, 10, 15); qr(1, 6, 11, 12); qr(2, 7, 8, 13); qr(3, 4, 9, 14);
    }
    for (int i = 0; i < 16; ++i) out[i] = x[i] + init[i];
}
}  // namespace

StdRng::StdRng(const std::array<uint8_t, 32>& seed) { memcpy(key_, seed.data(), 32); }
StdRng StdRng::from_os_entropy() {
    std::array<uint8_t, 32> seed{};
    FILE* f = fopen("/dev/urandom", "rb");
    if (!f || fread(seed.data(), 1, 32, f) != 32) {
        if (f) fclose(f);
        throw Error(ZKHIP_ERR_DEVICE, "cannot read /dev/urandom");
    }
    fclose(f);
    return StdRng(seed);
}
uint32_t StdRng::next_u32() {
    if (index_ >= 16) {
        chacha_block(key_, counter_++, 0, 12, block_);
        index_ = 0;
    }
    return block_[index_++];
}
uint64_t StdRng::next_u64() {
    const uint64_t lo = next_u32();
    return lo | ((uint64_t)next_u32() << 32);
}
StdRng get_rng_from_entropy(const std::string& entropy) {
    const std::array<uint8_t, 64> h = blake2b_512((const uint8_t*)entropy.data(), entropy.size());
    std::array<uint8_t, 32> seed;
    memcpy(seed.data(), h.data(), 32);
    return StdRng(seed);
}

// ------------------------------------------------------------------ Fr::rand
namespace {
struct FrParams {
    uint64_t p[4];
    int shave;            // REPR_SHAVE_BITS = 256 - modulus bits
};
const FrParams FR_BN128 = {{0x43e1f593f0000001ull, 0x2833e84879b97091ull, 0xb85045b68181585dull, 0x30644e72e131a029ull}, 2};
const FrParams FR_BLS12_381 = {{0xffffffff00000001ull, 0x53bda402fffe5bfeull, 0x3339d80809a1d805ull, 0x73eda753299d7d48ull}, 1};
const FrParams FR_BLS12_377 = {{0x0a11800000000001ull, 0x59aa76fed0000001ull, 0x60b44d1e5c37b001ull, 0x12ab655e9a2ca556ull}, 3};
const char* curve_name(int32_t curve) {
    if (curve == ZKHIP_CURVE_BN128) return "bn128";
    if (curve == ZKHIP_CURVE_BLS12_381) return "bls12_381";
    if (curve == ZKHIP_CURVE_BLS12_377) return "bls12_377";
    throw Error(ZKHIP_ERR_BAD_ARG, "unknown curve id");
}
bool known_curve(int32_t curve) { return curve == ZKHIP_CURVE_BN128 || curve == ZKHIP_CURVE_BLS12_381 || curve == ZKHIP_CURVE_BLS12_377; }
bool lt(const uint64_t a[4], const uint64_t b[4]) {
    for (int i = 3; i >= 0; --i)
        if (a[i] != b[i]) return a[i] < b[i];
    return false;
}
// x * 2^-256 mod p (Montgomery reduction of a 256-bit value: the limbs ark samples ARE the Montgomery representation)
void from_mont(const uint64_t x[4], const FrParams& f, uint64_t out[4]) {
    uint64_t inv = 1;                                             // -p^-1 mod 2^64 by Newton iteration
    for (int i = 0; i < 6; ++i) inv *= 2 - f.p[0] * inv;
    inv = (uint64_t)0 - inv;
    uint64_t t[5] = {x[0], x[1], x[2], x[3], 0};
    for (int i = 0; i < 4; ++i) {
        const uint64_t m = t[0] * inv;
        unsigned __int128 c = (unsigned __int128)m * f.p[0] + t[0];
        c >>= 64;
        for (int j = 1; j < 4; ++j) {
            c += (unsigned __int128)m * f.p[j] + t[j];
            t[j - 1] = (uint64_t)c;
            c >>= 64;
        }
        c += t[4];
        t[3] = (uint64_t)c;
        t[4] = (uint64_t)(c >> 64);
    }
    if (t[4] || !lt(t, f.p)) {                                    // one conditional subtraction
        unsigned __int128 b = 0;
        for (int j = 0; j < 4; ++j) {
            const unsigned __int128 d = (unsigned __int128)t[j] - f.p[j] - (uint64_t)b;
            t[j] = (uint64_t)d;
            b = (d >> 64) & 1;
        }
    }
    memcpy(out, t, 32);
}
}  // namespace

std::array<uint8_t, 32> fr_rand(StdRng& rng, int32_t curve) {
    if (!known_curve(curve)) throw Error(ZKHIP_ERR_BAD_ARG, "unknown curve id");
    const FrParams& f = curve == ZKHIP_CURVE_BN128 ? FR_BN128 : curve == ZKHIP_CURVE_BLS12_381 ? FR_BLS12_381 : FR_BLS12_377;   // (known_curve: one of the three)
    for (;;) {
        uint64_t limbs[4];
        for (int i = 0; i < 4; ++i) limbs[i] = rng.next_u64();
        limbs[3] &= ~(uint64_t)0 >> f.shave;
        if (!lt(limbs, f.p)) continue;
        uint64_t canon[4];
        from_mont(limbs, f, canon);
        std::array<uint8_t, 32> out;
        memcpy(out.data(), canon, 32);
        return out;
    }
}

// ------------------------------------------------------------------ handles
Key::~Key() { if (pk_) zkhip_pk_free(pk_); }
Key& Key::operator=(Key&& o) noexcept {
    if (this != &o) {
        if (pk_) zkhip_pk_free(pk_);
        pk_ = o.pk_;
        o.pk_ = nullptr;
    }
    return *this;
}
Program::Program(const uint8_t* bytes, size_t len) {
    const int32_t rc = zkhip_prog_parse(bytes, len, &prog_);
    if (rc != ZKHIP_OK) throw Error(rc, zkhip_last_error(nullptr));
    uint64_t d[8];
    zkhip_prog_dims(prog_, d);
    curve_ = (int32_t)d[0]; n_ = d[1]; l_ = d[2]; w_ = d[3];
    inputs_ = d[4] + d[5];
}
Program::~Program() { if (prog_) zkhip_prog_free(prog_); }
std::string Program::row_variables(int32_t which, uint64_t row) const {
    const uint64_t* rp = nullptr;
    const uint32_t* col = nullptr;
    const uint8_t* val = nullptr;
    const int64_t* ids = nullptr;
    if (row >= n_ || zkhip_prog_matrix(prog_, which, &rp, &col, &val) != ZKHIP_OK || zkhip_prog_variable_order(prog_, &ids) != ZKHIP_OK) return "";
    std::string s;
    for (uint64_t q = rp[row]; q < rp[row + 1]; ++q) {
        const int64_t id = ids[col[q]];
        if (!s.empty()) s += " + ";
        s += id == 0 ? std::string("~one") : id > 0 ? "_" + std::to_string(id - 1) : "~out_" + std::to_string(-id - 1);
    }
    return s.empty() ? "0" : s;
}

Hip::Hip(int32_t device) {
    const int32_t rc = zkhip_ctx_create(device, &ctx_);
    if (rc != ZKHIP_OK) throw Error(rc, zkhip_last_error(nullptr));
}
Hip::~Hip() { if (ctx_) zkhip_ctx_free(ctx_); }
void Hip::init(int32_t hw_queues) {
    const int32_t rc = zkhip_init(hw_queues);
    if (rc != ZKHIP_OK) throw Error(rc, zkhip_last_error(nullptr));
}
// One proof, then the process ends: no window-multiple tables (ten times what they would save one proof), and every kernel on the
// context's one stream — the ~20 streams a resident prover overlaps its proofs on cost ~10 ms of queue set-up each, ~90 ms of a
// process whose proof takes 25 (profiles/r5_cli_start_profile.txt).
void Hip::one_shot() {
    check(zkhip_ctx_tune(ctx_, ZKHIP_TUNE_MSM_SETS, 64));
    check(zkhip_ctx_tune(ctx_, ZKHIP_TUNE_SERIAL, 1));
}
// A long-lived prover of LARGE DENSE circuits (accumulation-bound: 2^20 constraints and more): all sixteen streams of the context made
// in one go at its first proof, every accumulation lane type on a hardware dispatcher of its own and the fold chains on the fourth
// (core.cuh make_pipe_streams).  Measured per workload (profiles/r6t_*, r6w_*): +1-3 % proofs/s and a lone proof 0.25-0.4 ms sooner
// there, 5-15 % slower on thin circuits (SHA-256, Poseidon on BLS12-381, GM17) — so it is a request, never a default.
void Hip::separate_dispatchers() { check(zkhip_ctx_tune(ctx_, ZKHIP_TUNE_PIPE_PLAN, 1)); }
void Hip::check(int32_t rc) const {
    if (rc != ZKHIP_OK) throw Error(rc, zkhip_last_error(ctx_));
}
std::string Hip::describe() const {
    char buf[256];
    check(zkhip_describe(ctx_, buf, sizeof(buf)));
    return buf;
}
Key Hip::load_proving_key(Scheme scheme, int32_t curve, const uint8_t* bytes, size_t len) {
    Key k;
    check(scheme == Scheme::GM17 ? zkhip_pk_load_gm17(ctx_, curve, bytes, len, &k.pk_) : zkhip_pk_load_g16(ctx_, curve, bytes, len, &k.pk_));
    return k;
}
Key Hip::import_key_image(const uint8_t* bytes, size_t len) {
    Key k;
    check(zkhip_pk_import(ctx_, bytes, len, &k.pk_));
    return k;
}
std::vector<uint8_t> Hip::export_key_image(const Key& key) const {
    uint64_t size = 0;
    check(zkhip_pk_export_size(key.get(), &size));
    std::vector<uint8_t> out(size);
    check(zkhip_pk_export(key.get(), out.data(), size));
    return out;
}

// ------------------------------------------------------------------ proof points and JSON
namespace {
std::string hex_be(const uint8_t* le, size_t n) {
    static const char* D = "0123456789abcdef";
    std::string s = "0x";
    s.reserve(2 + 2 * n);
    for (size_t i = n; i-- > 0;) { s.push_back(D[le[i] >> 4]); s.push_back(D[le[i] & 15]); }
    return s;
}
double ms_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}
}  // namespace

System::~System() {
    if (plan_) zkhip_wplan_free(plan_);
    if (cs_) zkhip_r1cs_free(cs_);
}
System& System::operator=(System&& o) noexcept {
    if (this != &o) {
        if (plan_) zkhip_wplan_free(plan_);
        if (cs_) zkhip_r1cs_free(cs_);
        cs_ = o.cs_; prog_ = o.prog_; plan_ = o.plan_; plan_tried_ = o.plan_tried_; plan_why_ = std::move(o.plan_why_);
        o.cs_ = nullptr; o.prog_ = nullptr; o.plan_ = nullptr;
    }
    return *this;
}
// the System's plan, made on first use.  ZKHIP_ERR_BAD_ARG from zkhip_wplan_create is the library refusing the PROGRAM (or a pending
// context: then nothing is remembered and the next call tries again); anything else is an error like any other
zkhip_wplan* Hip::plan_of(const System& system) const {
    if (system.plan_ || system.plan_tried_) return system.plan_;
    const int32_t rc = zkhip_wplan_create(ctx_, system.program().get(), system.get(), &system.plan_);
    if (rc == ZKHIP_ERR_BAD_ARG) {
        system.plan_why_ = zkhip_last_error(ctx_);
        system.plan_tried_ = system.plan_why_.find("pending") == std::string::npos && system.plan_why_.find("queue is open") == std::string::npos;
        return nullptr;
    }
    check(rc);
    system.plan_tried_ = true;
    return system.plan_;
}
System Hip::load_system(const Program& program) {
    System s;
    check(zkhip_prog_r1cs_load(ctx_, program.get(), &s.cs_));
    s.prog_ = &program;
    return s;
}
bool Hip::bind(Key& key, const System& system) {
    const int32_t rc = zkhip_pk_bind_r1cs(ctx_, key.get(), system.get());
    if (rc == ZKHIP_ERR_NOMEM) return false;
    check(rc);
    return true;
}
bool Hip::is_bound(const Key& key, const System& system) const { return zkhip_pk_is_bound(key.get(), system.get()) == 1; }
bool Hip::set_checked(bool on) { return zkhip_ctx_set_checked(ctx_, on ? 1 : 0) == 1; }
bool Hip::checked() const { return zkhip_ctx_set_checked(ctx_, -1) == 1; }
bool Hip::check(const System& system, const uint8_t* witness, size_t witness_len, uint64_t* first_row, uint64_t* n_bad) {
    const Program& program = system.program();
    std::vector<uint8_t> z(program.variables() * 32);
    int32_t rc = zkhip_prog_assignment(program.get(), witness, witness_len, z.data(), nullptr, 0, nullptr);
    if (rc != ZKHIP_OK) throw Error(rc, zkhip_last_error(nullptr));
    rc = zkhip_r1cs_check(ctx_, system.get(), z.data(), nullptr, first_row, n_bad);
    if (rc != ZKHIP_ERR_UNSATISFIED) check(rc);
    return rc == ZKHIP_OK;
}

Proof Hip::prove(Scheme scheme, const Program& program, const uint8_t* witness, size_t witness_len, const Key& key, StdRng& rng, Timings* tm) {
    // the constraint system on the device, for this one proof
    auto t0 = std::chrono::steady_clock::now();
    const System system = load_system(program);
    const double upload = ms_since(t0);
    Proof p = prove(scheme, system, witness, witness_len, key, rng, tm);
    if (tm) tm->r1cs_upload = upload;
    return p;
}

namespace {
// (1) of a proof: the assignment in ark order and the public inputs as the ark backend computes them (groth16.rs:33-38).  `compact`:
// the witness straight into the packed form; packed when that is less than half of the plain bytes, else widened on the host
struct WitnessBytes {
    std::vector<uint8_t> z, packed, inputs;
    uint64_t n_inputs = 0, packed_len = 0;
    bool use_packed = false;
};
WitnessBytes read_witness(const Program& program, const uint8_t* witness, size_t witness_len, bool compact) {
    WitnessBytes w;
    const uint64_t m = program.variables();
    const uint64_t cap = witness_len / 40 + 2;
    w.inputs.resize(cap * 32);
    int32_t rc;
    if (compact) {
        uint64_t bound = 0;
        zkhip_assignment_pack_bound(m, &bound);
        w.packed.resize(bound);
        rc = zkhip_prog_assignment_packed(program.get(), witness, witness_len, w.packed.data(), bound, &w.packed_len, w.inputs.data(), cap, &w.n_inputs);
        if (rc != ZKHIP_OK) throw Error(rc, zkhip_last_error(nullptr));
        w.use_packed = 2 * w.packed_len < 32 * m;
        if (!w.use_packed) {
            w.z.resize(m * 32);
            uint64_t got = 0;
            rc = zkhip_assignment_unpack(w.packed.data(), w.packed_len, w.z.data(), m, &got);
            if (rc != ZKHIP_OK) throw Error(rc, zkhip_last_error(nullptr));
        }
    } else {
        w.z.resize(m * 32);
        rc = zkhip_prog_assignment(program.get(), witness, witness_len, w.z.data(), w.inputs.data(), cap, &w.n_inputs);
        if (rc != ZKHIP_OK) throw Error(rc, zkhip_last_error(nullptr));
    }
    return w;
}
// (3) the blinding scalars: the first draws ark makes from the caller's RNG — d1, d2, r (GM17) or r, s (Groth16)
void draw_rnd(Scheme scheme, int32_t curve, StdRng& rng, uint8_t rnd[96]) {
    for (int i = 0; i < (scheme == Scheme::GM17 ? 3 : 2); ++i) memcpy(rnd + 32 * i, fr_rand(rng, curve).data(), 32);
}
// (5) raw little-endian coordinates -> big-endian hex; a point at infinity is printed as ark's zero() = (0, 1)
Proof proof_from_raw(Scheme scheme, int32_t curve, std::vector<uint8_t>& raw, const uint8_t* inputs, uint64_t n_inputs) {
    const size_t fq = curve == ZKHIP_CURVE_BN128 ? 32 : 48;
    std::vector<uint8_t> one(fq, 0);
    one[0] = 1;
    if (raw[8 * fq]) memcpy(&raw[fq], one.data(), fq);
    if (raw[8 * fq + 1]) memcpy(&raw[4 * fq], one.data(), fq);
    if (raw[8 * fq + 2]) memcpy(&raw[7 * fq], one.data(), fq);
    Proof p;
    p.scheme = scheme == Scheme::GM17 ? "gm17" : "g16";
    p.curve = curve_name(curve);
    p.proof.a = {hex_be(&raw[0], fq), hex_be(&raw[fq], fq)};
    p.proof.b.x = {hex_be(&raw[2 * fq], fq), hex_be(&raw[3 * fq], fq)};
    p.proof.b.y = {hex_be(&raw[4 * fq], fq), hex_be(&raw[5 * fq], fq)};
    p.proof.c = {hex_be(&raw[6 * fq], fq), hex_be(&raw[7 * fq], fq)};
    for (uint64_t i = 0; i < n_inputs; ++i) p.inputs.push_back(hex_be(&inputs[32 * i], 32));
    return p;
}
}  // namespace

Proof Hip::prove(Scheme scheme, const System& system, const uint8_t* witness, size_t witness_len, const Key& key, StdRng& rng, Timings* tm) {
    const Program& program = system.program();
    const int32_t curve = program.curve();
    const size_t fq = curve == ZKHIP_CURVE_BN128 ? 32 : 48;
    // (1) the assignment and the public inputs
    auto t0 = std::chrono::steady_clock::now();
    last_packed_ = false;
    last_on_device_ = false;
    struct Resident {      // the witness on the device before the proof: widened from the packed form, or ordered from the file's bytes
        zkhip_assignment* a = nullptr;
        ~Resident() { if (a) zkhip_assignment_free(a); }
    } resident;
    zkhip_wplan* plan = device_witness_ && !compact_ ? plan_of(system) : nullptr;
    WitnessBytes w;
    if (plan) {
        w.inputs.resize(program.public_inputs() * 32);
        check(zkhip_assignment_upload_witness(ctx_, plan, witness, witness_len, w.inputs.data(), program.public_inputs(), &w.n_inputs, &resident.a));
        last_on_device_ = true;
    } else {
        w = read_witness(program, witness, witness_len, compact_);
    }
    last_packed_ = w.use_packed;
    if (tm) tm->witness_to_assignment = ms_since(t0);
    // (2) the constraint system: resident
    zkhip_r1cs* cs = system.get();
    if (tm) tm->r1cs_upload = 0;
    // (3) the blinding scalars; (4) the GPU
    t0 = std::chrono::steady_clock::now();
    std::vector<uint8_t> raw(8 * fq + 3);
    if (last_packed_) check(zkhip_assignment_upload_packed(ctx_, cs, w.packed.data(), w.packed_len, &resident.a));
    uint8_t rnd[96];
    draw_rnd(scheme, curve, rng, rnd);
    int32_t rc;
    if (scheme == Scheme::GM17) {
        rc = resident.a ? zkhip_prove_gm17_resident(ctx_, key.get(), cs, resident.a, rnd, raw.data(), nullptr)
                          : zkhip_prove_gm17(ctx_, key.get(), cs, w.z.data(), rnd, raw.data(), nullptr);
    } else {
        rc = resident.a ? zkhip_prove_g16_resident(ctx_, key.get(), cs, resident.a, rnd, rnd + 32, raw.data(), nullptr)
                          : zkhip_prove_g16(ctx_, key.get(), cs, w.z.data(), rnd, rnd + 32, raw.data(), nullptr);
    }
    check(rc);
    if (tm) tm->prove = ms_since(t0);
    return proof_from_raw(scheme, curve, raw, w.inputs.data(), w.n_inputs);
}

// ------------------------------------------------------------------ witnesses computed on the device
ExecPlan::~ExecPlan() { if (plan_) zkhip_xplan_free(plan_); }
ExecPlan& ExecPlan::operator=(ExecPlan&& o) noexcept {
    if (this != &o) {
        if (plan_) zkhip_xplan_free(plan_);
        plan_ = o.plan_; system_ = o.system_; memcpy(dims_, o.dims_, sizeof dims_);
        o.plan_ = nullptr;
    }
    return *this;
}
ExecPlan Hip::load_exec_plan(const System& system, const uint8_t* program_bytes, size_t program_len) {
    ExecPlan p;
    check(zkhip_xplan_create(ctx_, system.program().get(), system.get(), program_bytes, program_len, &p.plan_));
    p.system_ = &system;
    check(zkhip_xplan_dims(p.plan_, p.dims_));
    return p;
}
void Hip::set_exec_wide(bool on) { check(zkhip_ctx_tune(ctx_, ZKHIP_TUNE_EXEC_WIDE, on ? 1 : 0)); }
std::vector<ComputedWitness> Hip::compute_witness(const ExecPlan& plan, const uint8_t* args, uint32_t count, bool want_files) {
    std::vector<ComputedWitness> out(count);
    if (!count) return out;
    const uint64_t fb = plan.witness_bytes(), ni = plan.system().program().public_inputs();
    std::vector<zkhip_assignment*> handles(count, nullptr);
    std::vector<uint8_t> files(want_files ? (size_t)count * fb : 0), inputs((size_t)count * ni * 32 + 1);
    std::vector<int32_t> status(count);
    std::vector<uint64_t> st(count), row(count);
    const int32_t rc = zkhip_compute_witness(ctx_, plan.get(), count, args, handles.data(), want_files ? files.data() : nullptr, fb, inputs.data(), ni, status.data(),
                                             st.data(), row.data());
    for (uint32_t i = 0; i < count; ++i) out[i].z = handles[i];      // (owned from here on, whatever the return code)
    if (rc != ZKHIP_ERR_UNSATISFIED) check(rc);
    for (uint32_t i = 0; i < count; ++i) {
        out[i].satisfied = status[i] == ZKHIP_OK;
        out[i].first_statement = st[i];
        out[i].first_row = row[i];
        if (!out[i].satisfied) continue;
        if (want_files) out[i].file.assign(files.begin() + (size_t)i * fb, files.begin() + (size_t)(i + 1) * fb);
        out[i].inputs.assign(inputs.begin() + (size_t)i * ni * 32, inputs.begin() + (size_t)(i + 1) * ni * 32);
    }
    return out;
}
Proof Hip::prove(Scheme scheme, const System& system, const ComputedWitness& witness, const Key& key, StdRng& rng, Timings* tm) {
    if (!witness.satisfied || !witness.z) throw Error(ZKHIP_ERR_UNSATISFIED, "this instance did not satisfy its program: there is no assignment to prove from");
    const int32_t curve = system.program().curve();
    const size_t fq = curve == ZKHIP_CURVE_BN128 ? 32 : 48;
    last_packed_ = false;
    last_on_device_ = true;
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<uint8_t> raw(8 * fq + 3);
    uint8_t rnd[96];
    draw_rnd(scheme, curve, rng, rnd);
    check(scheme == Scheme::GM17 ? zkhip_prove_gm17_resident(ctx_, key.get(), system.get(), witness.z, rnd, raw.data(), nullptr)
                                 : zkhip_prove_g16_resident(ctx_, key.get(), system.get(), witness.z, rnd, rnd + 32, raw.data(), nullptr));
    if (tm) { tm->witness_to_assignment = 0; tm->r1cs_upload = 0; tm->prove = ms_since(t0); }
    return proof_from_raw(scheme, curve, raw, witness.inputs.data(), witness.inputs.size() / 32);
}

// ------------------------------------------------------------------ the proof queue (zkhip.h "proof queue")
Queue Hip::open_queue(Scheme scheme, const System& system, const Key& key) {
    Queue q;
    q.plan_ = device_witness_ ? plan_of(system) : nullptr;      // (before the queue is open: the plan's tables are copied in)
    check(zkhip_queue_open(ctx_, key.get(), system.get(), &q.q_));
    q.hip_ = this;
    q.prog_ = &system.program();
    q.scheme_ = scheme;
    return q;
}
Queue::~Queue() { close(); }
Queue::Queue(Queue&& o) noexcept
    : q_(o.q_), hip_(o.hip_), prog_(o.prog_), scheme_(o.scheme_), last_packed_(o.last_packed_), last_on_device_(o.last_on_device_), plan_(o.plan_),
      inputs_(std::move(o.inputs_)), on_device_(std::move(o.on_device_)) { o.q_ = nullptr; }
Queue& Queue::operator=(Queue&& o) noexcept {
    if (this != &o) {
        close();
        q_ = o.q_; hip_ = o.hip_; prog_ = o.prog_; scheme_ = o.scheme_; last_packed_ = o.last_packed_;
        last_on_device_ = o.last_on_device_; plan_ = o.plan_;
        inputs_ = std::move(o.inputs_);
        on_device_ = std::move(o.on_device_);
        o.q_ = nullptr;
    }
    return *this;
}
void Queue::close() {
    if (q_) zkhip_queue_close(q_);
    q_ = nullptr;
    inputs_.clear();
    on_device_.clear();
}
uint32_t Queue::capacity() const {
    uint32_t cap = 0;
    if (q_) zkhip_queue_state(q_, &cap, nullptr);
    return cap;
}
uint32_t Queue::in_flight() const {
    uint32_t n = 0;
    if (q_) zkhip_queue_state(q_, nullptr, &n);
    return n;
}
uint64_t Queue::submit(const uint8_t* witness, size_t witness_len, StdRng& rng) {
    if (!q_) throw Error(ZKHIP_ERR_BAD_ARG, "the queue is closed");
    if (full()) throw Error(ZKHIP_ERR_BUSY, "the proof queue is full: collect a proof first");      // (before the RNG is touched)
    const int32_t curve = prog_->curve();
    uint8_t rnd[96];
    uint64_t ticket = 0;
    if (plan_ && !hip_->compact_) {      // the file's bytes as they are: the device tests, orders and checks them, and returns the inputs
        draw_rnd(scheme_, curve, rng, rnd);
        hip_->check(zkhip_queue_submit_witness(q_, plan_, witness, witness_len, rnd, &ticket));
        last_packed_ = false;
        last_on_device_ = true;
        inputs_.emplace_back();
        on_device_.push_back(true);
        return ticket;
    }
    WitnessBytes w = read_witness(*prog_, witness, witness_len, hip_->compact_);
    draw_rnd(scheme_, curve, rng, rnd);
    // the buffers are the library's copies when the call returns: `w` may go
    hip_->check(w.use_packed ? zkhip_queue_submit_packed(q_, w.packed.data(), w.packed_len, rnd, &ticket) : zkhip_queue_submit(q_, w.z.data(), nullptr, rnd, &ticket));
    last_packed_ = w.use_packed;
    last_on_device_ = false;
    w.inputs.resize(w.n_inputs * 32);
    inputs_.push_back(std::move(w.inputs));
    on_device_.push_back(false);
    return ticket;
}
bool Queue::ready() {
    int32_t r = 0;
    if (!q_) return false;
    hip_->check(zkhip_queue_ready(q_, &r));
    return r != 0;
}
Proof Queue::collect(uint64_t* ticket) {
    if (!q_) throw Error(ZKHIP_ERR_BAD_ARG, "the queue is closed");
    const int32_t curve = prog_->curve();
    std::vector<uint8_t> raw(8 * (curve == ZKHIP_CURVE_BN128 ? 32 : 48) + 3);
    uint64_t t = 0;
    const bool had = in_flight() > 0;
    const bool device = had && !on_device_.empty() && on_device_.front();
    std::vector<uint8_t> from_device(device ? prog_->public_inputs() * 32 : 0);
    uint64_t n_device = 0;
    const int32_t rc = device ? zkhip_queue_collect_inputs(q_, &t, raw.data(), from_device.data(), prog_->public_inputs(), &n_device, nullptr)
                              : zkhip_queue_collect(q_, &t, raw.data(), nullptr);
    std::vector<uint8_t> inputs;
    if (had && !inputs_.empty()) {      // (its ticket is spent whether the proof came out or not)
        inputs = std::move(inputs_.front());
        inputs_.erase(inputs_.begin());
        on_device_.erase(on_device_.begin());
    }
    hip_->check(rc);
    if (device) {
        from_device.resize(n_device * 32);
        inputs = std::move(from_device);
    }
    if (ticket) *ticket = t;
    return proof_from_raw(scheme_, curve, raw, inputs.data(), inputs.size() / 32);
}

// ------------------------------------------------------------------ setup
namespace {
std::string json_g1(const uint8_t* p, size_t fq, const std::string& ind) {
    std::vector<uint8_t> t(p, p + 2 * fq);
    t[2 * fq - 1] &= 0x3f;                                   // ark's flag bits live in the last byte
    return "[\n" + ind + "  \"" + hex_be(&t[0], fq) + "\",\n" + ind + "  \"" + hex_be(&t[fq], fq) + "\"\n" + ind + "]";
}
std::string json_g2(const uint8_t* p, size_t fq, const std::string& ind) {
    std::vector<uint8_t> t(p, p + 4 * fq);
    t[4 * fq - 1] &= 0x3f;
    auto pair = [&](size_t k) {
        return "[\n" + ind + "    \"" + hex_be(&t[k * fq], fq) + "\",\n" + ind + "    \"" + hex_be(&t[(k + 1) * fq], fq) + "\"\n" + ind + "  ]";
    };
    return "[\n" + ind + "  " + pair(0) + ",\n" + ind + "  " + pair(2) + "\n" + ind + "]";
}
std::string json_g1_list(const uint8_t* p, uint64_t count, size_t fq) {
    if (!count) return "[]";
    std::string s = "[\n";
    for (uint64_t i = 0; i < count; ++i) s += "    " + json_g1(p + i * 2 * fq, fq, "    ") + (i + 1 < count ? ",\n" : "\n");
    return s + "  ]";
}
}  // namespace

SetupKeypair Hip::setup(Scheme scheme, const Program& program, StdRng& rng) {
    const int32_t curve = program.curve();
    std::array<uint8_t, 32> tox[5];
    for (int k = 0; k < 5;) {                                   // alpha, beta, gamma, delta, tau: redrawn while zero
        tox[k] = fr_rand(rng, curve);
        bool zero = true;
        for (uint8_t b : tox[k]) zero = zero && b == 0;
        if (!zero) ++k;
    }
    zkhip_r1cs* cs = nullptr;
    check(zkhip_prog_r1cs_load(ctx_, program.get(), &cs));
    SetupKeypair kp;
    uint64_t size = 0;
    int32_t rc;
    if (scheme == Scheme::GM17) {
        uint8_t t4[128];
        memcpy(t4, tox[0].data(), 32); memcpy(t4 + 32, tox[1].data(), 32);
        memset(t4 + 64, 0, 32); t4[64] = 1;                     // ark-gm17's generate_random_parameters: gamma = 1
        memcpy(t4 + 96, tox[4].data(), 32);
        zkhip_setup_gm17_size(cs, &size);
        kp.pk.resize(size);
        rc = zkhip_setup_gm17(ctx_, cs, t4, nullptr, nullptr, kp.pk.data(), size);
    } else {
        uint8_t t5[160];
        for (int k = 0; k < 5; ++k) memcpy(t5 + 32 * k, tox[k].data(), 32);
        zkhip_setup_g16_size(cs, &size);
        kp.pk.resize(size);
        rc = zkhip_setup_g16(ctx_, cs, t5, nullptr, nullptr, kp.pk.data(), size);
    }
    zkhip_r1cs_free(cs);
    check(rc);
    kp.vk = verification_key_json(scheme, curve, kp.pk.data(), kp.pk.size());
    return kp;
}

// The verification key sits at the head of ark's proving key (ProvingKey { vk, .. }: serialize_unchecked writes it first):
// g16: alpha_g1, beta_g2, gamma_g2, delta_g2, gamma_abc_g1[]; gm17: h_g2, g_alpha_g1, h_beta_g2, g_gamma_g1, h_gamma_g2, query[].
std::string verification_key_json(Scheme scheme, int32_t curve, const uint8_t* pk, size_t len) {
    if (!known_curve(curve)) throw Error(ZKHIP_ERR_BAD_ARG, "verification_key_json: unsupported curve");
    const size_t fq = curve == ZKHIP_CURVE_BN128 ? 32 : 48, g1 = 2 * fq, g2 = 4 * fq;
    const size_t fixed = scheme == Scheme::GM17 ? 2 * g1 + 3 * g2 : g1 + 3 * g2;
    if (!pk || len < fixed + 8) throw Error(ZKHIP_ERR_PARSE, "proving key too short for its verification key");
    uint64_t count;
    memcpy(&count, pk + fixed, 8);
    if (count > (len - fixed - 8) / g1) throw Error(ZKHIP_ERR_PARSE, "proving key too short for its verification key");
    const std::string cname = curve_name(curve);
    std::string s = "{\n";
    if (scheme == Scheme::GM17) {      // (scheme/gm17.rs:19-27)
        size_t pos = 0;
        const uint8_t *h = pk; pos += g2;
        const uint8_t* g_alpha = pk + pos; pos += g1;
        const uint8_t* h_beta = pk + pos; pos += g2;
        const uint8_t* g_gamma = pk + pos; pos += g1;
        const uint8_t* h_gamma = pk + pos; pos += g2;
        s += "  \"scheme\": \"gm17\",\n  \"curve\": \"" + cname + "\",\n";
        s += "  \"h\": " + json_g2(h, fq, "  ") + ",\n  \"g_alpha\": " + json_g1(g_alpha, fq, "  ") + ",\n  \"h_beta\": " + json_g2(h_beta, fq, "  ") + ",\n";
        s += "  \"g_gamma\": " + json_g1(g_gamma, fq, "  ") + ",\n  \"h_gamma\": " + json_g2(h_gamma, fq, "  ") + ",\n";
        s += "  \"query\": " + json_g1_list(pk + pos + 8, count, fq) + "\n}";
    } else {                           // (scheme/groth16.rs:18-25)
        s += "  \"scheme\": \"g16\",\n  \"curve\": \"" + cname + "\",\n";
        s += "  \"alpha\": " + json_g1(pk, fq, "  ") + ",\n  \"beta\": " + json_g2(pk + g1, fq, "  ") + ",\n";
        s += "  \"gamma\": " + json_g2(pk + g1 + g2, fq, "  ") + ",\n  \"delta\": " + json_g2(pk + g1 + 2 * g2, fq, "  ") + ",\n";
        s += "  \"gamma_abc\": " + json_g1_list(pk + fixed + 8, count, fq) + "\n}";
    }
    return s;
}


Proof Hip::generate_proof(Scheme scheme, const uint8_t* program, size_t program_len, const uint8_t* witness, size_t witness_len,
                          const uint8_t* proving_key, size_t proving_key_len, StdRng& rng) {
    Program prog(program, program_len);
    Key key = load_proving_key(scheme, prog.curve(), proving_key, proving_key_len);
    return prove(scheme, prog, witness, witness_len, key, rng);
}

std::string Proof::to_json() const {
    std::string s;
    auto str = [](const std::string& v) { return "\"" + v + "\""; };
    auto g1 = [&](const G1Affine& p, const std::string& ind) {
        return "[\n" + ind + "  " + str(p.x) + ",\n" + ind + "  " + str(p.y) + "\n" + ind + "]";
    };
    auto pair = [&](const std::array<std::string, 2>& c, const std::string& ind) {
        return "[\n" + ind + "  " + str(c[0]) + ",\n" + ind + "  " + str(c[1]) + "\n" + ind + "]";
    };
    s += "{\n";
    s += "  \"scheme\": " + str(scheme) + ",\n";
    s += "  \"curve\": " + str(curve) + ",\n";
    s += "  \"proof\": {\n";
    s += "    \"a\": " + g1(proof.a, "    ") + ",\n";
    s += "    \"b\": [\n      " + pair(proof.b.x, "      ") + ",\n      " + pair(proof.b.y, "      ") + "\n    ],\n";
    s += "    \"c\": " + g1(proof.c, "    ") + "\n";
    s += "  },\n";
    if (inputs.empty()) {
        s += "  \"inputs\": []\n";
    } else {
        s += "  \"inputs\": [\n";
        for (size_t i = 0; i < inputs.size(); ++i) s += "    " + str(inputs[i]) + (i + 1 < inputs.size() ? ",\n" : "\n");
        s += "  ]\n";
    }
    s += "}";
    return s;
}

}  // namespace zokrates_hip
