// zkhip_backend.hpp — the host side of the `hip` proving backend in C++, above the C ABI of zkhip.h.
//
// The reference's host side is Rust: `impl Backend<T, G16> for Ark` / `impl Backend<T, GM17> for Ark`
// (/root/reference/zokrates_ark/src/groth16.rs:20-53, gm17.rs:43-78) behind the trait of
// /root/reference/zokrates_proof_systems/src/lib.rs:98-112, driven by `zokrates generate-proof`
// (/root/reference/zokrates_cli/src/ops/generate_proof.rs:95-202).  No Rust toolchain exists in this image, so the
// compiled host layer is C++ with the same names, argument meaning and error behaviour:
//
//   reference                                              here
//   Backend::generate_proof(program, witness, pk, rng)     Hip::generate_proof(scheme, program, witness, pk, rng)
//   Proof { proof: ProofPoints { a, b, c }, inputs }       Proof / ProofPoints / G1Affine / G2Affine   (lib.rs:33-96, scheme/groth16.rs:8-16)
//   TaggedProof -> serde_json::to_string_pretty            Proof::to_json()                            (tagged.rs:14-37)
//   Backend::verify(vk, proof) -> bool                     verify(VerificationKey, Proof) -> bool      (groth16.rs:55-87, gm17.rs:69-110; host CPU)
//   get_rng_from_entropy(&str) -> StdRng                   get_rng_from_entropy(std::string) -> StdRng (rng.rs:5-20)
//   StdRng::from_entropy()                                 StdRng::from_os_entropy()
//   panic!(..) on any failure (groth16.rs:41-44 unwrap)    throws zokrates_hip::Error (code = ZKHIP_ERR_*, message of the library)
//
// `program` and `witness` are the bytes of ZoKrates' own files (`out`, `witness`): the walk of
// `Computation::generate_constraints` (zokrates_ark/src/lib.rs:80-129) and `public_inputs_values` happen inside
// zkhip_prog_parse / zkhip_prog_assignment.  The Rust adapter that would sit behind the real trait is
// integration/zokrates_hip (source only); this layer is what is compiled, tested and shipped here (tools: zkhip-cli).
#pragma once
#include <array>
#include <cstring>
#include <cstdint>
#include <map>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "zkhip.h"

namespace zokrates_hip {

enum class Scheme { G16, GM17 };

struct Error : std::runtime_error {
    int32_t code;
    Error(int32_t c, const std::string& m) : std::runtime_error(m), code(c) {}
};

// "0x" + lower-case hex, big-endian, zero-padded to the base-field width (parse_g1 / parse_g2: zokrates_ark/src/lib.rs:150-218)
struct G1Affine { std::string x, y; };
struct G2Affine { std::array<std::string, 2> x, y; };   // (c0, c1)
struct ProofPoints { G1Affine a; G2Affine b; G1Affine c; };
struct Proof {
    std::string scheme, curve;            // the tags of TaggedProof
    ProofPoints proof;
    std::vector<std::string> inputs;      // public_inputs_values as 32-byte big-endian hex (parse_fr, lib.rs:220-226)
    std::string to_json() const;          // serde_json::to_string_pretty of the tagged proof: the text of proof.json
    static Proof from_json(const std::string& text);      // serde_json::from_value::<Proof<T, S>> (ops/verify.rs:181-182); Error on a malformed file
    // `zokrates print-proof --format json|remix` (ops/print_proof.rs:85-114): the line to paste into the Solidity verifier; bn128 only
    std::string print(const std::string& format) const;
};

// `verification.key` (scheme/groth16.rs:18-25: alpha, beta, gamma, delta, gamma_abc; scheme/gm17.rs:19-27: h, g_alpha, h_beta,
// g_gamma, h_gamma, query), points as in the file, looked up by the file's field names
struct VerificationKey {
    std::string scheme, curve;
    std::map<std::string, G1Affine> g1;
    std::map<std::string, G2Affine> g2;
    std::vector<G1Affine> query;          // gamma_abc (g16) / query (gm17)
    static VerificationKey from_json(const std::string& text);
};

// Backend<T, S>::verify(vk, proof) -> bool (zokrates_ark/src/groth16.rs:55-87, gm17.rs:69-110): the pairing check, on the host
// CPU as in the reference (no GPU, no context; csrc/host/verify.cpp).  bn128, bls12_381 and — for the reference's own golden proofs —
// bls12_377; g16 and gm17.  false: the equation
// does not hold, or a point is off its curve / outside the r-torsion.  Error: curve or scheme of the two files differ (the CLI's
// messages, ops/verify.rs:95-107), a coordinate or input is not canonical, the input count does not fit the key (the reference
// panics through `unwrap` there).
bool verify(const VerificationKey& vk, const Proof& proof);
// The same check on the device, for batches (Hip::load_verification_key, Hip::verify_batch below; csrc/pairing.cuh).  The host
// `verify` stays and stays the default.  What crosses the C ABI, made from the hex strings with the host verifier's strictness:
// the key in ark's `serialize_unchecked` byte layout (every coordinate "0x" + exactly the field's width, else Error; a coordinate
// that is not below the modulus is refused where the key is loaded), a proof as the 8 x sz(Fq) + 3 byte record of zkhip_prove_g16 / _gm17, its inputs as 32-byte little-endian words
// (defined inline at the end of this header, with the two Hip methods: a program that links the host layer without them pays nothing)
std::vector<uint8_t> verification_key_bytes(const VerificationKey& vk);
std::vector<uint8_t> proof_record(const Proof& proof);
std::vector<uint8_t> proof_inputs(const Proof& proof);
// a verifying key resident on the GPU (zkhip_vk): made by Hip::load_verification_key, freed with the object
class DeviceVerificationKey {
  public:
    DeviceVerificationKey() = default;
    DeviceVerificationKey(DeviceVerificationKey&& o) noexcept { *this = std::move(o); }
    DeviceVerificationKey& operator=(DeviceVerificationKey&& o) noexcept {
        std::swap(vk_, o.vk_); std::swap(scheme_, o.scheme_); std::swap(curve_, o.curve_); std::swap(inputs_, o.inputs_);
        return *this;
    }
    DeviceVerificationKey(const DeviceVerificationKey&) = delete;
    DeviceVerificationKey& operator=(const DeviceVerificationKey&) = delete;
    ~DeviceVerificationKey();
    const std::string& scheme() const { return scheme_; }
    const std::string& curve() const { return curve_; }
    uint64_t inputs() const { return inputs_; }

  private:
    friend class Hip;
    zkhip_vk* vk_ = nullptr;
    std::string scheme_, curve_;
    uint64_t inputs_ = 0;
};
// the text of `verification.key` for the key at the head of an ark proving key (ProvingKey { vk, .. }); Error if the bytes are too short
std::string verification_key_json(Scheme scheme, int32_t curve, const uint8_t* proving_key, size_t len);
// prod_i e(g1_i, g2_i) == 1 in the target group (the Solidity verifier's `pairing` precompile call, solidity.rs:  pairingProd*)
bool pairing_product_is_one(const std::string& curve, const std::vector<std::pair<G1Affine, G2Affine>>& pairs);

// rand 0.8.5 `StdRng` (= rand_chacha 0.3.1 ChaCha12Rng): key = seed, 64-bit block counter, words of a block in order
class StdRng {
  public:
    explicit StdRng(const std::array<uint8_t, 32>& seed);
    static StdRng from_os_entropy();      // StdRng::from_entropy(): 32 bytes of /dev/urandom
    uint32_t next_u32();
    uint64_t next_u64();                  // two consecutive words, low first (rand_core BlockRng)

  private:
    uint32_t key_[8];
    uint64_t counter_ = 0;
    uint32_t block_[16];
    int index_ = 16;
};
// zokrates_proof_systems::rng::get_rng_from_entropy: seed = first 32 bytes of Blake2b-512(entropy)
StdRng get_rng_from_entropy(const std::string& entropy);
std::array<uint8_t, 64> blake2b_512(const uint8_t* data, size_t len);
// ark-ff 0.3.0 `Fr::rand(rng)` as 32 canonical little-endian bytes (curve: ZKHIP_CURVE_*)
std::array<uint8_t, 32> fr_rand(StdRng& rng, int32_t curve);

// A proving key resident on the GPU (ProvingKey::deserialize_unchecked + the MSM tables: zkhip_pk_load_* / zkhip_pk_import)
class Key {
  public:
    Key() = default;
    ~Key();
    Key(Key&& o) noexcept : pk_(o.pk_) { o.pk_ = nullptr; }
    Key& operator=(Key&& o) noexcept;
    Key(const Key&) = delete;
    Key& operator=(const Key&) = delete;
    zkhip_pk* get() const { return pk_; }
    explicit operator bool() const { return pk_ != nullptr; }

  private:
    friend class Hip;
    zkhip_pk* pk_ = nullptr;
};

// A compiled program (`out`) decoded into the R1CS in ark variable order (host side only: zkhip_prog_parse)
class Program {
  public:
    Program(const uint8_t* bytes, size_t len);     // ProgEnum::deserialize + Computation::generate_constraints' variable walk
    ~Program();
    Program(const Program&) = delete;
    Program& operator=(const Program&) = delete;
    int32_t curve() const { return curve_; }
    uint64_t constraints() const { return n_; }
    uint64_t variables() const { return l_ + w_; }
    uint64_t public_inputs() const { return inputs_; }     // public arguments + return count: the length of a proof's `inputs`
    zkhip_prog* get() const { return prog_; }
    // the ZoKrates names ("~one", "_7", "~out_0": zkhip_prog_variable_order) of the variables in row `row` of A (0), B (1) or C (2),
    // joined by " + " — what a failing constraint index (Hip::check) is worth to the author of the program
    std::string row_variables(int32_t which, uint64_t row) const;

  private:
    zkhip_prog* prog_ = nullptr;
    int32_t curve_ = 0;
    uint64_t n_ = 0, l_ = 0, w_ = 0, inputs_ = 0;
};

// A program's constraint system resident on the GPU (zkhip_prog_r1cs_load).  `Backend::generate_proof` consumes its program
// and the one-call form below uploads the system for every proof, as the reference rebuilds its ConstraintSystem for every proof
// (zokrates_ark/src/lib.rs:80-129); a caller that proves many witnesses of one program — zokrates_js calls generate_proof many
// times per process, zokrates_js/src/lib.rs:380-452 — keeps a System next to its Key and may bind the two (Hip::bind).
class System {
  public:
    System() = default;
    ~System();
    System(System&& o) noexcept : cs_(o.cs_), prog_(o.prog_), plan_(o.plan_), plan_tried_(o.plan_tried_), plan_why_(std::move(o.plan_why_)) {
        o.cs_ = nullptr; o.prog_ = nullptr; o.plan_ = nullptr;
    }
    System& operator=(System&& o) noexcept;
    System(const System&) = delete;
    System& operator=(const System&) = delete;
    zkhip_r1cs* get() const { return cs_; }
    const Program& program() const { return *prog_; }     // (the Program must outlive the System)

  private:
    friend class Hip;
    zkhip_r1cs* cs_ = nullptr;
    const Program* prog_ = nullptr;
    // the program's column order on the device (zkhip_wplan_create), made the first time a proof wants it (Hip::set_device_witness);
    // stays null — with the library's reason in plan_why_ — for a program the plan refuses, which keeps the host reader
    mutable zkhip_wplan* plan_ = nullptr;
    mutable bool plan_tried_ = false;
    mutable std::string plan_why_;
};

// A program's statements compiled for the device (zkhip.h "witnesses computed on the device": zkhip_xplan_create), for
// Hip::compute_witness.  Made from the System and the bytes of the `out` file its Program was parsed from; the System must outlive it.
class ExecPlan {
  public:
    ExecPlan() = default;
    ~ExecPlan();
    ExecPlan(ExecPlan&& o) noexcept : plan_(o.plan_), system_(o.system_) { memcpy(dims_, o.dims_, sizeof dims_); o.plan_ = nullptr; }
    ExecPlan& operator=(ExecPlan&& o) noexcept;
    ExecPlan(const ExecPlan&) = delete;
    ExecPlan& operator=(const ExecPlan&) = delete;
    zkhip_xplan* get() const { return plan_; }
    const System& system() const { return *system_; }
    uint64_t arguments() const { return dims_[0]; }
    uint64_t statements() const { return dims_[1]; }
    uint64_t witness_bytes() const { return 8 + 40 * dims_[5]; }      // the length of the program's `witness` file
    uint64_t store_bytes_per_instance() const { return dims_[7]; }
    explicit operator bool() const { return plan_ != nullptr; }

  private:
    friend class Hip;
    zkhip_xplan* plan_ = nullptr;
    const System* system_ = nullptr;
    uint64_t dims_[8] = {0, 0, 0, 0, 0, 0, 0, 0};
};
// One instance of Hip::compute_witness: the reference's `witness` bytes (if asked for), public_inputs_values, and the assignment
// resident on the device for Hip::prove — or, for an instance that failed a check, the statement of the `out` file and the R1CS row.
struct ComputedWitness {
    bool satisfied = false;
    uint64_t first_statement = 0, first_row = 0;      // (of a failed instance)
    std::vector<uint8_t> file, inputs;                // inputs: 32-byte LE values
    zkhip_assignment* z = nullptr;
    ComputedWitness() = default;
    ~ComputedWitness() { if (z) zkhip_assignment_free(z); }
    ComputedWitness(ComputedWitness&& o) noexcept : satisfied(o.satisfied), first_statement(o.first_statement), first_row(o.first_row), file(std::move(o.file)),
                                                   inputs(std::move(o.inputs)), z(o.z) { o.z = nullptr; }
    ComputedWitness& operator=(ComputedWitness&& o) noexcept {
        if (this != &o) { if (z) zkhip_assignment_free(z); satisfied = o.satisfied; first_statement = o.first_statement; first_row = o.first_row;
                          file = std::move(o.file); inputs = std::move(o.inputs); z = o.z; o.z = nullptr; }
        return *this;
    }
    ComputedWitness(const ComputedWitness&) = delete;
    ComputedWitness& operator=(const ComputedWitness&) = delete;
};

// NonUniversalBackend::setup's result (zokrates_proof_systems/src/lib.rs:59-65,113-118): the verification key as the text of
// `verification.key` (scheme/groth16.rs:18-25, scheme/gm17.rs:19-27) and the proving key in ark's serialize_unchecked bytes
struct SetupKeypair {
    std::string vk;
    std::vector<uint8_t> pk;
};

// where the wall clock of one proof went (milliseconds)
struct Timings {
    double witness_to_assignment = 0, r1cs_upload = 0, prove = 0;
};

class Hip;
// Witnesses that arrive ONE AT A TIME, proved at the rate of a batch (zkhip.h "proof queue"): up to capacity() proofs of one resident
// (System, Key) in flight across calls.  submit() reads the witness, draws the blinding scalars from the caller's RNG in the order
// Hip::prove draws them (so equal seeds give equal proofs, whatever the order of submit and collect) and returns without waiting for
// the device; collect() returns the OLDEST proof.  It honours Hip::set_compact_witness with prove()'s rule — a witness whose packed form
// is less than half of the m x 32 B goes to the device packed (zkhip_queue_submit_packed) — and, where that is off,
// Hip::set_device_witness as it stood when the queue was opened (zkhip_queue_submit_witness; the inputs then come back with the proof).
// While a Queue is open its Hip refuses
// every other proving call (zkhip.h, Conventions); close() — or the destructor — drops what is uncollected.  The Hip, the System and
// the Key must outlive it.  An Error from collect() concerns that one proof (its ticket is spent); the others stay in flight.
class Queue {
  public:
    Queue() = default;
    ~Queue();
    Queue(Queue&& o) noexcept;
    Queue& operator=(Queue&& o) noexcept;
    Queue(const Queue&) = delete;
    Queue& operator=(const Queue&) = delete;
    uint32_t capacity() const;
    uint32_t in_flight() const;
    bool full() const { return in_flight() >= capacity(); }
    uint64_t submit(const uint8_t* witness, size_t witness_len, StdRng& rng);      // the ticket; Error(ZKHIP_ERR_BUSY) when full
    bool ready();                                                                  // would collect() return without waiting?  Never blocks
    Proof collect(uint64_t* ticket = nullptr);
    bool last_witness_packed() const { return last_packed_; }
    bool last_witness_on_device() const { return last_on_device_; }
    void close();
    explicit operator bool() const { return q_ != nullptr; }

  private:
    friend class Hip;
    zkhip_queue* q_ = nullptr;
    const Hip* hip_ = nullptr;
    const Program* prog_ = nullptr;
    Scheme scheme_ = Scheme::G16;
    bool last_packed_ = false, last_on_device_ = false;
    zkhip_wplan* plan_ = nullptr;                   // the System's, when the Hip's device-witness setting was on at open_queue and the plan exists
    std::vector<std::vector<uint8_t>> inputs_;      // public_inputs_values of the tickets in flight, oldest first (empty: the device has them)
    std::vector<bool> on_device_;                   // which of those tickets were submitted as witness files
};

// One GPU.  (The reference's backends are unit structs — `pub struct Ark;` — because they own nothing; this one owns a
// zkhip_ctx, so it is an object.  Not re-entrant, like the context.)
class Hip {
  public:
    explicit Hip(int32_t device = 0);
    ~Hip();
    // Process-wide, BEFORE the first Hip object (and before any other HIP user of the process starts the runtime): ask the HIP
    // runtime for `hw_queues` hardware queues (zkhip_init).  A resident prover keeps ~20 streams busy and wants 8 (16 if it is the
    // only context of its process); a one-proof process runs on one stream and need not call this.  The library never changes the
    // process environment on its own.
    static void init(int32_t hw_queues = 8);
    // One proof per process (what `generate-proof` is): keys loaded from now on skip the precomputed window multiples — building
    // them costs ten times what they save a single proof (0.15 s of kernels at 2^20 against ~5 ms of proof time) — and the MSMs
    // fold one bucket set per window instead (ZKHIP_TUNE_MSM_SETS).  A resident prover keeps the default.
    void one_shot();
    // A long-lived prover, before its first proof: the context's streams made in one go and placed on the GPU's four dispatchers by
    // plan (ZKHIP_TUNE_PIPE_PLAN; sixteen streams: call init(16) first, and keep the process below ~22 hardware queues in all).  Level
    // or better than streams in order of first use on every measured workload; not for one-proof processes (0.15 s).
    void separate_dispatchers();
    Hip(const Hip&) = delete;
    Hip& operator=(const Hip&) = delete;

    // Backend<T, S>::generate_proof(program, witness, proving_key, rng) -> Proof, on the bytes of the three files
    Proof generate_proof(Scheme scheme, const uint8_t* program, size_t program_len, const uint8_t* witness, size_t witness_len,
                         const uint8_t* proving_key, size_t proving_key_len, StdRng& rng);

    // the same in its parts, for callers that keep keys resident, cache their device layout or overlap the steps
    Key load_proving_key(Scheme scheme, int32_t curve, const uint8_t* bytes, size_t len);
    Key import_key_image(const uint8_t* bytes, size_t len);            // zkhip_pk_import
    std::vector<uint8_t> export_key_image(const Key& key) const;      // zkhip_pk_export (compact: level 0 of the tables)
    Proof prove(Scheme scheme, const Program& program, const uint8_t* witness, size_t witness_len, const Key& key, StdRng& rng,
                Timings* timings = nullptr);
    // a long-lived prover: the constraint system uploaded once, the key (Groth16 or GM17) bound to it (zkhip_pk_bind_r1cs: the quotient's
    // inverse transforms applied to the key's bases once, four transforms per proof afterwards, the same proof).  bind returns
    // false when the device has no room for the two extra tables: the key then proves as it was loaded.
    System load_system(const Program& program);
    bool bind(Key& key, const System& system);
    bool is_bound(const Key& key, const System& system) const;
    Proof prove(Scheme scheme, const System& system, const uint8_t* witness, size_t witness_len, const Key& key, StdRng& rng,
                Timings* timings = nullptr);
    // NonUniversalBackend<T, S>::setup(program, rng) -> SetupKeypair: toxic waste = five non-zero `Fr::rand` draws (alpha, beta,
    // gamma, delta, tau; GM17: gamma = 1 as in ark-gm17), standard group generators (ark samples random ones from the RNG: a
    // key made here is valid, not byte-equal to `zokrates setup --entropy`'s), key generation on the GPU (zkhip_setup_*)
    SetupKeypair setup(Scheme scheme, const Program& program, StdRng& rng);
    // Checked proving (zkhip.h "checked proving").  check: does the witness satisfy the system?  On the device, without a key
    // (zkhip_r1cs_check); false fills *first_row (the statement number of the `out` file) and *n_bad where given.  set_checked:
    // every prove of this object tests its assignment on the device and throws Error(ZKHIP_ERR_UNSATISFIED, "... constraint k ...")
    // instead of returning a proof that cannot verify; off by default, returns the previous setting.
    bool check(const System& system, const uint8_t* witness, size_t witness_len, uint64_t* first_row = nullptr, uint64_t* n_bad = nullptr);
    bool set_checked(bool on);
    bool checked() const;
    // Compact witnesses (zkhip.h "compact assignments"): prove() reads the witness straight into the packed form
    // (zkhip_prog_assignment_packed) and, when that is less than half of the m x 32 B (a witness of bits and small integers), uploads
    // it packed and proves through the resident entry point; a dense witness takes the usual path.  The same proof either way;
    // off by default.  Returns the previous setting; last_witness_packed() says which way the last prove() went.
    bool set_compact_witness(bool on) { const bool was = compact_; compact_ = on; return was; }
    bool last_witness_packed() const { return last_packed_; }
    // Witness files on the device (zkhip.h "witness files on the device"): prove(System, ..) and Queue::submit hand the file's bytes
    // to the device, which tests, orders and checks them (zkhip_assignment_upload_witness / zkhip_queue_submit_witness) — no host pass
    // over the entries.  The System owns the plan, made on first use (a Queue: when it is opened, so set this before open_queue).
    // Where zkhip_wplan_create refuses the program (a repeated parameter, an output without a column) the host reader is used as
    // before and last_witness_on_device() says so.  The blinding scalars are drawn in the same order either way: equal seeds give
    // equal Proofs.  set_compact_witness wins if both are set.  One difference in what is accepted: zkhip.h names it (entries for
    // variables the program lacks are ignored).  Off by default; returns the previous setting.
    bool set_device_witness(bool on) { const bool was = device_witness_; device_witness_ = on; return was; }
    bool last_witness_on_device() const { return last_on_device_; }
    // Witnesses computed on the device (zkhip.h "witnesses computed on the device"): what `zokrates compute-witness` does on one host
    // thread, for a BATCH of argument lists in one launch.  load_exec_plan compiles the statements of `program_bytes` (the `out` file
    // the System's Program was parsed from) and throws Error(ZKHIP_ERR_BAD_ARG, "... keeps the host interpreter") for a program the
    // device does not run (asm blocks, the bellman SHA round, the in-circuit verifier).  compute_witness takes count x arguments x 32
    // bytes (canonical LE) and returns one ComputedWitness per instance; an instance that fails a check comes back with satisfied =
    // false and the others are delivered.  A lone instance runs on one lane: the route pays in batches.  prove() over a
    // ComputedWitness proves from its resident assignment: the same Proof as prove() over its `file`.
    ExecPlan load_exec_plan(const System& system, const uint8_t* program_bytes, size_t program_len);
    std::vector<ComputedWitness> compute_witness(const ExecPlan& plan, const uint8_t* args, uint32_t count, bool want_files = true);
    // A lone witness across the device (ZKHIP_TUNE_EXEC_WIDE): compute_witness runs the program's dependency levels, one work-item per
    // (instruction of a level, instance), instead of one per instance — the route for one request or a few.  The same results; off
    // by default.  Throws under a pending split proof, like every tunable.
    void set_exec_wide(bool on);
    Proof prove(Scheme scheme, const System& system, const ComputedWitness& witness, const Key& key, StdRng& rng, Timings* timings = nullptr);
    // a long-lived prover fed one witness at a time: a proof queue over a resident system and key (see Queue above)
    Queue open_queue(Scheme scheme, const System& system, const Key& key);
    std::string describe() const;

    // Backend::verify on the device (zkhip_vk_load_*, zkhip_verify_*_batch): the key's points are tested and prepared once; then one
    // verdict per proof, the host `verify`'s for every proof on which it answers; where it throws for a proof (tags that differ from
    // the key's, an input count that does not fit it, a coordinate or input that is not canonical) this throws, naming the proof
    DeviceVerificationKey load_verification_key(const VerificationKey& vk);
    std::vector<bool> verify_batch(const DeviceVerificationKey& vk, const std::vector<Proof>& proofs);

  private:
    friend class Queue;
    zkhip_ctx* ctx_ = nullptr;
    bool compact_ = false, last_packed_ = false;
    bool device_witness_ = false, last_on_device_ = false;
    zkhip_wplan* plan_of(const System& system) const;      // the System's plan, made on first use; null if the program is refused
    void check(int32_t rc) const;
};

// ---------------- verification on the device: what crosses the C ABI, and the two Hip methods ----------------
namespace detail {      // not part of the interface: the spelling of points and fields on either side of the C ABI
inline size_t fq_bytes_of(const std::string& curve) {
    if (curve == "bn128") return 32;
    if (curve == "bls12_381" || curve == "bls12_377") return 48;
    throw Error(ZKHIP_ERR_BAD_ARG, "verify: curve " + curve + " is not supported (bn128, bls12_381, bls12_377)");
}
// "0x" + exactly 2 nb hex digits, big-endian -> nb bytes, little-endian, appended
inline void hex_to_le(const std::string& s, size_t nb, std::vector<uint8_t>& out) {
    if (s.size() != 2 + 2 * nb || s[0] != '0' || s[1] != 'x')
        throw Error(ZKHIP_ERR_PARSE, "verify: a coordinate must be \"0x\" followed by " + std::to_string(2 * nb) + " hex digits, got \"" + s + "\"");
    const size_t at = out.size();
    out.resize(at + nb, 0);
    for (size_t i = 2; i < s.size(); ++i) {
        const char c = s[i];
        const int h = c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10 : c >= 'A' && c <= 'F' ? c - 'A' + 10 : -1;
        if (h < 0) throw Error(ZKHIP_ERR_PARSE, "verify: bad hex digit in \"" + s + "\"");
        const size_t nib = s.size() - 1 - i;
        out[at + nib / 2] |= (uint8_t)(h << (4 * (nib % 2)));
    }
}
inline void g1_le(const G1Affine& a, size_t nb, std::vector<uint8_t>& out) { hex_to_le(a.x, nb, out); hex_to_le(a.y, nb, out); }
inline void g2_le(const G2Affine& a, size_t nb, std::vector<uint8_t>& out) {
    hex_to_le(a.x[0], nb, out); hex_to_le(a.x[1], nb, out); hex_to_le(a.y[0], nb, out); hex_to_le(a.y[1], nb, out);
}
}  // namespace detail
inline std::vector<uint8_t> verification_key_bytes(const VerificationKey& vk) {
    const size_t nb = detail::fq_bytes_of(vk.curve);
    const bool g16 = vk.scheme == "g16";
    if (!g16 && vk.scheme != "gm17") throw Error(ZKHIP_ERR_BAD_ARG, "verify: scheme " + vk.scheme + " is not supported (g16, gm17)");
    std::vector<uint8_t> out;
    if (g16) {
        detail::g1_le(vk.g1.at("alpha"), nb, out); detail::g2_le(vk.g2.at("beta"), nb, out); detail::g2_le(vk.g2.at("gamma"), nb, out); detail::g2_le(vk.g2.at("delta"), nb, out);
    } else {
        detail::g2_le(vk.g2.at("h"), nb, out); detail::g1_le(vk.g1.at("g_alpha"), nb, out); detail::g2_le(vk.g2.at("h_beta"), nb, out); detail::g1_le(vk.g1.at("g_gamma"), nb, out);
        detail::g2_le(vk.g2.at("h_gamma"), nb, out);
    }
    const uint64_t n = vk.query.size();
    for (int i = 0; i < 8; ++i) out.push_back((uint8_t)(n >> (8 * i)));
    for (const auto& q : vk.query) detail::g1_le(q, nb, out);
    return out;
}
inline std::vector<uint8_t> proof_record(const Proof& proof) {
    const size_t nb = detail::fq_bytes_of(proof.curve);
    std::vector<uint8_t> out;
    detail::g1_le(proof.proof.a, nb, out); detail::g2_le(proof.proof.b, nb, out); detail::g1_le(proof.proof.c, nb, out);
    out.resize(out.size() + 3, 0);          // (a point at infinity has no spelling in proof.json)
    return out;
}
inline std::vector<uint8_t> proof_inputs(const Proof& proof) {
    std::vector<uint8_t> out;
    for (const std::string& s : proof.inputs) {
        size_t i = 0;
        while (s.compare(i, 2, "0x") == 0) i += 2;
        if (i == s.size()) throw Error(ZKHIP_ERR_PARSE, "verify: empty input \"" + s + "\"");
        while (i + 1 < s.size() && s[i] == '0') ++i;
        if (s.size() - i > 64) throw Error(ZKHIP_ERR_PARSE, "verify: input " + s + " is not below the scalar field modulus");
        detail::hex_to_le("0x" + std::string(64 - (s.size() - i), '0') + s.substr(i), 32, out);
    }
    return out;
}

inline DeviceVerificationKey::~DeviceVerificationKey() { if (vk_) zkhip_vk_free(vk_); }
namespace detail {
inline int32_t curve_id_of(const std::string& curve) {
    if (curve == "bn128") return ZKHIP_CURVE_BN128;
    if (curve == "bls12_381") return ZKHIP_CURVE_BLS12_381;
    if (curve == "bls12_377") return ZKHIP_CURVE_BLS12_377;
    throw Error(ZKHIP_ERR_BAD_ARG, "verify: curve " + curve + " is not supported (bn128, bls12_381, bls12_377)");
}
}  // namespace detail
inline DeviceVerificationKey Hip::load_verification_key(const VerificationKey& vk) {
    const std::vector<uint8_t> bytes = verification_key_bytes(vk);
    DeviceVerificationKey out;
    out.scheme_ = vk.scheme;
    out.curve_ = vk.curve;
    check((vk.scheme == "gm17" ? zkhip_vk_load_gm17 : zkhip_vk_load_g16)(ctx_, detail::curve_id_of(vk.curve), bytes.data(), bytes.size(), &out.vk_));
    uint64_t dims[2];
    check(zkhip_vk_dims(out.vk_, dims));
    out.inputs_ = dims[0];
    return out;
}
inline std::vector<bool> Hip::verify_batch(const DeviceVerificationKey& vk, const std::vector<Proof>& proofs) {
    if (!vk.vk_) throw Error(ZKHIP_ERR_BAD_ARG, "verify_batch: no verification key loaded");
    std::vector<uint8_t> recs, inputs;
    for (size_t i = 0; i < proofs.size(); ++i) {
        const Proof& p = proofs[i];
        const std::string at = "proof " + std::to_string(i) + ": ";
        if (p.curve != vk.curve_)
            throw Error(ZKHIP_ERR_BAD_ARG, at + "Expected the curve of the proof and the verification key to be equal, found " + p.curve + " != " + vk.curve_);
        if (p.scheme != vk.scheme_)
            throw Error(ZKHIP_ERR_BAD_ARG, at + "Expected the scheme of the proof and the verification key to be equal, found " + p.scheme + " != " + vk.scheme_);
        if (p.inputs.size() != vk.inputs_)
            throw Error(ZKHIP_ERR_BAD_ARG, at + "verify: " + std::to_string(p.inputs.size()) + " public inputs for a verification key made for " + std::to_string(vk.inputs_));
        try {
            const std::vector<uint8_t> r = proof_record(p), in = proof_inputs(p);
            recs.insert(recs.end(), r.begin(), r.end());
            inputs.insert(inputs.end(), in.begin(), in.end());
        } catch (const Error& e) {
            throw Error(e.code, at + e.what());
        }
    }
    std::vector<uint8_t> ok(proofs.size(), 0);
    const auto call = vk.scheme_ == "gm17" ? zkhip_verify_gm17_batch : zkhip_verify_g16_batch;
    check(call(ctx_, vk.vk_, proofs.size(), recs.data(), inputs.empty() ? nullptr : inputs.data(), ok.data()));
    return std::vector<bool>(ok.begin(), ok.end());
}
}  // namespace zokrates_hip
