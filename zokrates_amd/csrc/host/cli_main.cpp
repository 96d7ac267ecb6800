// zkhip-cli — `zokrates generate-proof` for the hip backend, as a native executable over zkhip_backend.hpp.
//
//   zkhip-cli generate-proof -i out -w witness -p proving.key -j proof.json [-s g16|gm17] [--entropy TEXT]
//                            [--key-cache DIR] [--device N] [--timings] [--verify [--device-verify]] [--check] [--compact-witness] [--device-witness]
//   zkhip-cli generate-proof -i out --arguments v1 v2 ... -p proving.key -j proof.json      (the witness computed on the device)
//   zkhip-cli compute-witness -i out -a v1 v2 ... -o witness [--verbose] [--wide] [--device N]
//
// Mirrors /root/reference/zokrates_cli/src/ops/generate_proof.rs:95-202: the compiled program (`out`), the witness and the
// proving key are read from files, the proof is written as JSON, one proof per process; `--entropy` seeds the RNG as
// `get_rng_from_entropy` does, otherwise the OS does (`StdRng::from_entropy`).  Failures print the message and exit 1 (the
// reference's panic hook and `exit(1)`: zokrates_cli/src/bin.rs:18-25,90-105).
// The three inputs are independent until the proof starts: the program is read and decoded on host threads (zkhip_prog_parse
// cuts the constraint section into parallel chunks) WHILE the key is uploaded and its window multiples are built on the GPU.
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <sys/syscall.h>
#include <unistd.h>

#include <chrono>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <memory>
#include <thread>

#include "../../../include/zkhip_backend.hpp"

using namespace zokrates_hip;

namespace {
// a file mapped read-only (the page cache is the buffer: nothing is copied, nothing is zero-filled first)
struct Mapped {
    const uint8_t* data = nullptr;
    size_t size = 0;
    Mapped() = default;
    explicit Mapped(const std::string& path) {
        const int fd = open(path.c_str(), O_RDONLY);
        if (fd < 0) throw Error(ZKHIP_ERR_BAD_ARG, "cannot open " + path);
        struct stat st;
        if (fstat(fd, &st) != 0) { close(fd); throw Error(ZKHIP_ERR_BAD_ARG, "cannot stat " + path); }
        size = (size_t)st.st_size;
        if (size) {
            void* p = mmap(nullptr, size, PROT_READ, MAP_PRIVATE | MAP_POPULATE, fd, 0);
            if (p == MAP_FAILED) { close(fd); throw Error(ZKHIP_ERR_NOMEM, "cannot map " + path); }
            data = (const uint8_t*)p;
        }
        close(fd);
    }
    Mapped(Mapped&& o) noexcept : data(o.data), size(o.size) { o.data = nullptr; o.size = 0; }
    Mapped& operator=(Mapped&& o) noexcept { std::swap(data, o.data); std::swap(size, o.size); return *this; }
    Mapped(const Mapped&) = delete;
    Mapped& operator=(const Mapped&) = delete;
    ~Mapped() { if (data) munmap((void*)data, size); }
};
double ms_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}
uint64_t fnv1a(const std::string& s) {
    uint64_t h = 1469598103934665603ull;
    for (unsigned char c : s) { h ^= c; h *= 1099511628211ull; }
    return h;
}
// the CPU this thread runs on and its NUMA node (for the record in --timings: the host-side stages — reading, decoding, the
// staging copies — depend on where the process sits relative to the GPU); -1 where the kernel does not say
std::pair<int, int> cpu_and_node() {
    unsigned cpu = 0, node = 0;
#ifdef SYS_getcpu
    if (syscall(SYS_getcpu, &cpu, &node, nullptr) == 0) return {(int)cpu, (int)node};
#endif
    return {-1, -1};
}
int usage() {
    fprintf(stderr, "usage: zkhip-cli generate-proof -i <out> -w <witness> -p <proving.key> -j <proof.json> [-s g16|gm17] [--entropy TEXT] "
                    "[--key-cache DIR] [--device N] [--timings] [--verify [--device-verify]] [--check] [--compact-witness] [--device-witness] [--full-tables]\n"
                    "       zkhip-cli generate-proof -i <out> --arguments v1 v2 ... -p <proving.key> -j <proof.json> [-s g16|gm17] [--entropy TEXT] [--wide] [--device N]\n"
                    "       zkhip-cli compute-witness -i <out> [-a v1 v2 ...] [-o <witness>] [--verbose] [--wide] [--device N]\n"
                    "       zkhip-cli setup -i <out> -p <proving.key> -v <verification.key> [-s g16|gm17] [--entropy TEXT] [--device N]\n"
                    "       zkhip-cli verify [-v <verification.key>] [-j <proof.json>] [--device] [--timings [--repeat N]]\n"
                    "       zkhip-cli print-proof [-j <proof.json>] [-f remix|json]\n");
    return 2;
}
}  // namespace

namespace {
// a decimal field element as 32 little-endian bytes, as the reference's `-a` takes them (T::try_from_dec_str,
// zokrates_cli/src/ops/compute_witness.rs:132-139); whether it is below r is the library's to say
std::array<uint8_t, 32> from_decimal(const std::string& s) {
    std::array<uint8_t, 32> v{};
    if (s.empty()) throw Error(ZKHIP_ERR_PARSE, "Could not parse argument: " + s);
    for (char ch : s) {
        if (ch < '0' || ch > '9') throw Error(ZKHIP_ERR_PARSE, "Could not parse argument: " + s);
        unsigned carry = (unsigned)(ch - '0');
        for (int i = 0; i < 32; ++i) { const unsigned t = v[i] * 10u + carry; v[i] = (uint8_t)t; carry = t >> 8; }
        if (carry) throw Error(ZKHIP_ERR_PARSE, "Could not parse argument: " + s);
    }
    return v;
}
std::string to_decimal(const uint8_t* le) {
    uint8_t v[32];
    memcpy(v, le, 32);
    std::string out;
    for (;;) {
        unsigned rem = 0;
        bool any = false;
        for (int i = 31; i >= 0; --i) { const unsigned t = rem * 256u + v[i]; v[i] = (uint8_t)(t / 10u); rem = t % 10u; any = any || v[i]; }
        out.push_back((char)('0' + rem));
        if (!any) break;
    }
    return std::string(out.rbegin(), out.rend());
}
// the values after -a / --arguments, up to the next option
std::vector<uint8_t> take_arguments(int argc, char** argv, int& i) {
    std::vector<uint8_t> out;
    while (i + 1 < argc && argv[i + 1][0] != '-') {
        const std::array<uint8_t, 32> v = from_decimal(argv[++i]);
        out.insert(out.end(), v.begin(), v.end());
    }
    return out;
}
// one instance through the device: the plan of the program, the arguments in, the witness out; an Error names what failed
ComputedWitness compute_one(Hip& hip, const System& system, const Mapped& prog_bytes, const std::vector<uint8_t>& args) {
    const ExecPlan plan = hip.load_exec_plan(system, prog_bytes.data, prog_bytes.size);
    if (args.size() != plan.arguments() * 32)
        throw Error(ZKHIP_ERR_BAD_ARG, "Execution failed: Program takes " + std::to_string(plan.arguments()) + " inputs but was passed " + std::to_string(args.size() / 32) + " values");
    std::vector<ComputedWitness> w = hip.compute_witness(plan, args.data(), 1);
    if (!w[0].satisfied)
        throw Error(ZKHIP_ERR_UNSATISFIED, "Execution failed: statement " + std::to_string(w[0].first_statement) + " of the program (constraint " + std::to_string(w[0].first_row) +
                                               ") is not satisfied; its right-hand side is over " + system.program().row_variables(2, w[0].first_row));
    return std::move(w[0]);
}
}  // namespace

// zkhip-cli compute-witness -i out -a v1 v2 ... -o witness [--verbose] [--wide] [--device N]
// (/root/reference/zokrates_cli/src/ops/compute_witness.rs:98-233 with raw arguments: "Computing witness...", with --verbose the return
// values as the JSON of a tuple of field elements, the `witness` file, "Witness file written to '..'".  --abi, --stdin, --json and
// --circom-witness are not built.)  The witness is computed on the device (Hip::compute_witness): one instance on one lane, or with --wide
// across the device, level by level (Hip::set_exec_wide) — the same file.
int cmd_compute_witness(int argc, char** argv) {
    std::string input = "out", output = "witness";
    std::vector<uint8_t> args;
    bool verbose = false, wide = false;
    int device = 0;
    try {
        for (int i = 2; i < argc; ++i) {
            const std::string a = argv[i];
            auto val = [&]() -> std::string { if (i + 1 >= argc) { usage(); exit(2); } return argv[++i]; };
            if (a == "-i" || a == "--input") input = val();
            else if (a == "-o" || a == "--output") output = val();
            else if (a == "-a" || a == "--arguments") args = take_arguments(argc, argv, i);
            else if (a == "--verbose") verbose = true;
            else if (a == "--wide") wide = true;
            else if (a == "--device") device = atoi(val().c_str());
            else return usage();
        }
        printf("Computing witness...\n");
        const Mapped prog_bytes(input);
        const Program program(prog_bytes.data, prog_bytes.size);
        Hip hip(device);
        hip.set_exec_wide(wide);
        const System system = hip.load_system(program);
        const ComputedWitness w = compute_one(hip, system, prog_bytes, args);
        if (verbose) {
            // witness.return_values(): ~out_0 .. ~out_{R-1}, the tail of the public inputs; R is the header's return count
            uint32_t returns = 0;
            memcpy(&returns, prog_bytes.data + 16, 4);
            const size_t n = w.inputs.size() / 32;
            std::string list;
            for (size_t k = n - std::min<size_t>(returns, n); k < n; ++k) list += (list.empty() ? "\"" : ",\"") + to_decimal(&w.inputs[32 * k]) + "\"";
            printf("\nWitness: \n[%s]\n\n", list.c_str());
        }
        std::ofstream o(output, std::ios::binary);
        if (!o) throw Error(ZKHIP_ERR_BAD_ARG, "Could not create " + output);
        o.write((const char*)w.file.data(), (std::streamsize)w.file.size());
        o.close();
        if (!o) throw Error(ZKHIP_ERR_BAD_ARG, "Could not save witness");
        printf("Witness file written to '%s'\n", output.c_str());
        return 0;
    } catch (const std::exception& e) {
        fprintf(stderr, "zkhip-cli: %s\n", e.what());
        return 1;
    }
}

// zkhip-cli setup -i out -p proving.key -v verification.key [-s g16|gm17] [--entropy TEXT] [--device N]
// (/root/reference/zokrates_cli/src/ops/setup.rs: program in, proving.key + verification.key out)
int cmd_setup(int argc, char** argv) {
    std::string input = "out", pk_path = "proving.key", vk_path = "verification.key", scheme_s = "g16", entropy;
    bool have_entropy = false;
    int device = 0;
    for (int i = 2; i < argc; ++i) {
        const std::string a = argv[i];
        auto val = [&]() -> std::string { if (i + 1 >= argc) { usage(); exit(2); } return argv[++i]; };
        if (a == "-i" || a == "--input") input = val();
        else if (a == "-p" || a == "--proving-key-path") pk_path = val();
        else if (a == "-v" || a == "--verification-key-path") vk_path = val();
        else if (a == "-s" || a == "--proving-scheme") scheme_s = val();
        else if (a == "--entropy") { entropy = val(); have_entropy = true; }
        else if (a == "--device") device = atoi(val().c_str());
        else return usage();
    }
    if (scheme_s != "g16" && scheme_s != "gm17") return usage();
    try {
        const Mapped prog_bytes(input);
        const Program program(prog_bytes.data, prog_bytes.size);
        Hip hip(device);
        StdRng rng = have_entropy ? get_rng_from_entropy(entropy) : StdRng::from_os_entropy();
        const SetupKeypair kp = hip.setup(scheme_s == "gm17" ? Scheme::GM17 : Scheme::G16, program, rng);
        std::ofstream o(pk_path, std::ios::binary);
        o.write((const char*)kp.pk.data(), (std::streamsize)kp.pk.size());
        std::ofstream v(vk_path);
        v << kp.vk;
        o.close();                      // (the stream state is only final once the buffers have been flushed)
        v.close();
        if (!o || !v) throw Error(ZKHIP_ERR_BAD_ARG, "cannot write the key files");
        printf("setup (%s): %llu constraints, %llu variables; wrote %s, %s\n", scheme_s.c_str(), (unsigned long long)program.constraints(),
               (unsigned long long)program.variables(), pk_path.c_str(), vk_path.c_str());
        return 0;
    } catch (const std::exception& e) {
        fprintf(stderr, "zkhip-cli: %s\n", e.what());
        return 1;
    }
}

static std::string slurp(const std::string& path) {
    std::ifstream f(path, std::ios::binary);
    if (!f) throw Error(ZKHIP_ERR_BAD_ARG, "Could not open " + path);
    return std::string((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

// zkhip-cli verify -v verification.key -j proof.json      (/root/reference/zokrates_cli/src/ops/verify.rs:49-195: curve and scheme
// come from the two files and must agree; "Performing verification..." then PASSED or FAILED, exit status 0 for both; no GPU)
int cmd_verify(int argc, char** argv) {
    std::string vk_path = "verification.key", proof_path = "proof.json";
    bool on_device = false, timings = false;
    int repeat = 1;
    for (int i = 2; i < argc; ++i) {
        const std::string a = argv[i];
        auto val = [&]() -> std::string { if (i + 1 >= argc) { usage(); exit(2); } return argv[++i]; };
        if (a == "-v" || a == "--verification-key-path") vk_path = val();
        else if (a == "-j" || a == "--proof-path") proof_path = val();
        else if (a == "-b" || a == "--backend") val();          // accepted and ignored: there is one verifier here
        else if (a == "--device") on_device = true;             // the pairing check on the GPU (Hip::verify_batch): the same text and status
        else if (a == "--timings") timings = true;              // a last line `timings {"verify_ms": [..]}`: the check alone, once per --repeat
        else if (a == "--repeat") repeat = std::max(1, atoi(val().c_str()));
        else return usage();
    }
    try {
        const VerificationKey vk = VerificationKey::from_json(slurp(vk_path));
        const Proof proof = Proof::from_json(slurp(proof_path));
        printf("Performing verification...\n");
        bool ok = false;
        std::vector<double> ms;
        if (on_device) {
            if (proof.curve != vk.curve)
                throw Error(ZKHIP_ERR_BAD_ARG, "Expected the curve of the proof and the verification key to be equal, found " + proof.curve + " != " + vk.curve);
            if (proof.scheme != vk.scheme)
                throw Error(ZKHIP_ERR_BAD_ARG, "Expected the scheme of the proof and the verification key to be equal, found " + proof.scheme + " != " + vk.scheme);
            Hip hip(0);
            const DeviceVerificationKey dvk = hip.load_verification_key(vk);
            for (int k = 0; k < repeat; ++k) {
                const auto t0 = std::chrono::steady_clock::now();
                ok = hip.verify_batch(dvk, {proof})[0];
                ms.push_back(ms_since(t0));
            }
        } else {
            for (int k = 0; k < repeat; ++k) {
                const auto t0 = std::chrono::steady_clock::now();
                ok = verify(vk, proof);
                ms.push_back(ms_since(t0));
            }
        }
        printf("%s\n", ok ? "PASSED" : "FAILED");
        if (timings) {
            std::string list;
            for (double v : ms) { char buf[32]; snprintf(buf, sizeof buf, "%s%.3f", list.empty() ? "" : ", ", v); list += buf; }
            printf("timings {\"verify_ms\": [%s]}\n", list.c_str());
        }
        return 0;
    } catch (const std::exception& e) {
        fprintf(stderr, "%s\n", e.what());
        return 1;
    }
}

// zkhip-cli print-proof -j proof.json -f remix|json       (zokrates_cli/src/ops/print_proof.rs)
int cmd_print_proof(int argc, char** argv) {
    std::string proof_path = "proof.json", format = "remix";
    for (int i = 2; i < argc; ++i) {
        const std::string a = argv[i];
        auto val = [&]() -> std::string { if (i + 1 >= argc) { usage(); exit(2); } return argv[++i]; };
        if (a == "-j" || a == "--proof-path") proof_path = val();
        else if (a == "-f" || a == "--format") format = val();
        else return usage();
    }
    try {
        fputs(Proof::from_json(slurp(proof_path)).print(format).c_str(), stdout);
        return 0;
    } catch (const std::exception& e) {
        fprintf(stderr, "%s\n", e.what());
        return 1;
    }
}

// zkhip-cli pairing-check <curve> <file>: the file holds lines "g1x g1y g2x0 g2x1 g2y0 g2y1" (hex as in proof.json); prints ONE or
// NOT-ONE for the product of the pairings (a test hook for the pairing itself: bilinearity on the reference's MPC fixture points)
int cmd_pairing_check(int argc, char** argv) {
    if (argc != 4) return usage();
    try {
        std::ifstream f(argv[3]);
        if (!f) throw Error(ZKHIP_ERR_BAD_ARG, std::string("Could not open ") + argv[3]);
        std::vector<std::pair<G1Affine, G2Affine>> pairs;
        std::string w[6];
        while (f >> w[0] >> w[1] >> w[2] >> w[3] >> w[4] >> w[5]) pairs.push_back({G1Affine{w[0], w[1]}, G2Affine{{w[2], w[3]}, {w[4], w[5]}}});
        printf("%s\n", pairing_product_is_one(argv[2], pairs) ? "ONE" : "NOT-ONE");
        return 0;
    } catch (const std::exception& e) {
        fprintf(stderr, "%s\n", e.what());
        return 1;
    }
}

int main(int argc, char** argv) {
    if (argc >= 2 && strcmp(argv[1], "setup") == 0) return cmd_setup(argc, argv);
    if (argc >= 2 && strcmp(argv[1], "verify") == 0) return cmd_verify(argc, argv);
    if (argc >= 2 && strcmp(argv[1], "compute-witness") == 0) return cmd_compute_witness(argc, argv);
    if (argc >= 2 && strcmp(argv[1], "print-proof") == 0) return cmd_print_proof(argc, argv);
    if (argc >= 2 && strcmp(argv[1], "pairing-check") == 0) return cmd_pairing_check(argc, argv);
    if (argc < 2 || strcmp(argv[1], "generate-proof") != 0) return usage();
    std::string input = "out", witness_path = "witness", pk_path = "proving.key", proof_path = "proof.json", scheme_s = "g16", entropy, cache_dir;
    bool have_entropy = false, timings = false, self_check = false, resident_tables = false, check_first = false, compact = false, device_witness = false, device_verify = false, wide = false;
    int device = 0;
    bool from_arguments = false;      // --arguments in place of -w: the witness computed on the device, the proof from its resident assignment
    std::vector<uint8_t> arguments;
    for (int i = 2; i < argc; ++i) {
        const std::string a = argv[i];
        auto val = [&]() -> std::string { if (i + 1 >= argc) { usage(); exit(2); } return argv[++i]; };
        if (a == "-i" || a == "--input") input = val();
        else if (a == "--arguments") {
            try { arguments = take_arguments(argc, argv, i); } catch (const Error& e) { fprintf(stderr, "zkhip-cli: %s\n", e.what()); return 1; }
            from_arguments = true;
        }
        else if (a == "--wide") wide = true;                         // with --arguments: the witness level by level across the device (the same proof.json)
        else if (a == "--verify") self_check = true;
        else if (a == "--device-verify") device_verify = true;   // with --verify: that check on the GPU (Hip::verify_batch) instead of the host CPU
        else if (a == "--check") check_first = true;                 // the witness against the constraints, on the device, before proving
        else if (a == "--compact-witness") compact = true;           // the witness packed on the host and widened on the device when that halves it
        else if (a == "--device-witness") device_witness = true;     // the witness file's bytes tested, ordered and checked on the device (the same proof.json)
        else if (a == "--full-tables") resident_tables = true;      // (measurement: build the window-multiple tables a resident prover uses)
        else if (a == "-w" || a == "--witness") witness_path = val();
        else if (a == "-p" || a == "--proving-key-path") pk_path = val();
        else if (a == "-j" || a == "--proof-path") proof_path = val();
        else if (a == "-s" || a == "--proving-scheme") scheme_s = val();
        else if (a == "--entropy") { entropy = val(); have_entropy = true; }
        else if (a == "--key-cache") cache_dir = val();
        else if (a == "--device") device = atoi(val().c_str());
        else if (a == "--timings") timings = true;
        else return usage();
    }
    if (scheme_s != "g16" && scheme_s != "gm17") return usage();
    const Scheme scheme = scheme_s == "gm17" ? Scheme::GM17 : Scheme::G16;
    const auto t_start = std::chrono::steady_clock::now();
    try {
        // host side, beside the key upload: read + decode the program, read the witness
        std::unique_ptr<Program> program;
        Mapped witness;
        std::string host_error;
        int32_t host_code = 0;
        double ms_read = 0, ms_parse = 0;
        std::thread host([&] {
            try {
                auto t0 = std::chrono::steady_clock::now();
                const Mapped prog_bytes(input);
                if (!from_arguments) witness = Mapped(witness_path);
                ms_read = ms_since(t0);
                t0 = std::chrono::steady_clock::now();
                program.reset(new Program(prog_bytes.data, prog_bytes.size));
                ms_parse = ms_since(t0);
            } catch (const Error& e) {
                host_error = e.what();
                host_code = e.code;
            } catch (const std::exception& e) {
                host_error = e.what();
                host_code = ZKHIP_ERR_NOMEM;
            }
        });
        struct Joiner { std::thread& t; ~Joiner() { if (t.joinable()) t.join(); } };
        Joiner joiner{host};
        // the curve of the key: bytes 8..12 of the program file (Field::id)
        int32_t curve = -1;
        {
            FILE* f = fopen(input.c_str(), "rb");
            uint8_t head[12] = {0};
            if (!f || fread(head, 1, 12, f) != 12) { if (f) fclose(f); throw Error(ZKHIP_ERR_PARSE, "Invalid header"); }
            fclose(f);
            static const uint8_t BN[4] = {0xb4, 0xf7, 0xb5, 0xbd}, BLS[4] = {0x40, 0xd8, 0xc1, 0xf9}, BLS377[4] = {0xc2, 0x95, 0x5a, 0xb5};
            curve = !memcmp(head + 8, BN, 4) ? ZKHIP_CURVE_BN128 : !memcmp(head + 8, BLS, 4) ? ZKHIP_CURVE_BLS12_381 : !memcmp(head + 8, BLS377, 4) ? ZKHIP_CURVE_BLS12_377 : -1;
            if (memcmp(head, "ZOK\0", 4) != 0 || curve < 0) throw Error(ZKHIP_ERR_PARSE, "not a ZoKrates program for bn128 / bls12_381 / bls12_377");
        }
        // which bytes hold the key (the image of an earlier run, if --key-cache has one): mapped on a second thread while the
        // HIP runtime starts
        std::string key_source = "proving.key", image_path;
        bool try_image = false;
        if (!cache_dir.empty()) {
            struct stat st;
            if (stat(pk_path.c_str(), &st) != 0) throw Error(ZKHIP_ERR_BAD_ARG, "cannot stat " + pk_path);
            char tag[64];
            snprintf(tag, sizeof(tag), "%016llx", (unsigned long long)fnv1a(pk_path + "|" + std::to_string((long long)st.st_size) + "|" +
                                                                           std::to_string((long long)st.st_mtim.tv_sec) + "." + std::to_string((long long)st.st_mtim.tv_nsec) + "|" +
                                                                           std::to_string((unsigned long long)st.st_ino) + "|" + scheme_s + "|" + std::to_string(curve) + (resident_tables ? "|tables" : "")));
            image_path = cache_dir + "/" + tag + ".zkhippk";
            struct stat ist;
            try_image = stat(image_path.c_str(), &ist) == 0;
        }
        Mapped key_bytes;
        std::string key_error;
        std::thread key_reader([&] {
            try {
                key_bytes = Mapped(try_image ? image_path : pk_path);
            } catch (const std::exception& e) {
                key_error = e.what();
            }
        });
        Joiner key_joiner{key_reader};
        auto t0 = std::chrono::steady_clock::now();
        Hip hip(device);
        if (!resident_tables) hip.one_shot();          // one proof, then the process ends: no window-multiple tables
        hip.set_compact_witness(compact);
        hip.set_device_witness(device_witness);
        const double ms_init = ms_since(t0);
        t0 = std::chrono::steady_clock::now();
        key_reader.join();
        if (!key_error.empty()) throw Error(ZKHIP_ERR_BAD_ARG, key_error);
        Key key;
        if (try_image) {
            try {
                key = hip.import_key_image(key_bytes.data, key_bytes.size);
                key_source = "image";
            } catch (const Error&) {
                key_bytes = Mapped(pk_path);                  // a stale image of another library build: rewrite it below
            }
        }
        if (!key) {
            key = hip.load_proving_key(scheme, curve, key_bytes.data, key_bytes.size);
            if (!image_path.empty()) {
                mkdir(cache_dir.c_str(), 0777);
                const std::vector<uint8_t> img = hip.export_key_image(key);
                const std::string tmp = image_path + ".tmp" + std::to_string((long long)getpid());
                std::ofstream o(tmp, std::ios::binary);
                o.write((const char*)img.data(), (std::streamsize)img.size());
                o.close();
                // only a completely written image enters the cache (ENOSPC, I/O error: the run goes on without one)
                if (!o || rename(tmp.c_str(), image_path.c_str()) != 0) {
                    unlink(tmp.c_str());
                    fprintf(stderr, "warning: key image not cached (%s could not be written)\n", image_path.c_str());
                }
            }
        }
        const double ms_key = ms_since(t0);
        t0 = std::chrono::steady_clock::now();
        host.join();
        const double ms_wait = ms_since(t0);
        if (!program) throw Error(host_code ? host_code : ZKHIP_ERR_PARSE, host_error);
        StdRng rng = have_entropy ? get_rng_from_entropy(entropy) : StdRng::from_os_entropy();
        Timings tm;
        // --check: Az o Bz == Cz on the device first (zkhip_r1cs_check: the three mat-vecs and one pointwise pass) — a witness that
        // fails is refused with the number of its first failing constraint, the statement number of the `out` file
        System system;
        double ms_check = 0;
        if (check_first && !from_arguments) {      // (a witness computed on the device has passed the program's own checks there)
            t0 = std::chrono::steady_clock::now();
            system = hip.load_system(*program);
            tm.r1cs_upload = ms_since(t0);
            t0 = std::chrono::steady_clock::now();
            uint64_t first_row = 0, n_bad = 0;
            if (!hip.check(system, witness.data, witness.size, &first_row, &n_bad))
                throw Error(ZKHIP_ERR_UNSATISFIED, "the witness does not satisfy the program: constraint " + std::to_string(first_row) + " of " +
                                                       std::to_string(program->constraints()) + " is not satisfied (" + std::to_string(n_bad) +
                                                       " in all); its right-hand side is over " + program->row_variables(2, first_row));
            ms_check = ms_since(t0);
            printf("checked: the witness satisfies all %llu constraints (%.3f ms)\n", (unsigned long long)program->constraints(), ms_check);
        }
        const double upload_ms = tm.r1cs_upload;
        Proof proof;
        if (from_arguments) {
            // the statements run on the device (one instance: one lane, or --wide), the proof from the assignment they leave there
            hip.set_exec_wide(wide);
            t0 = std::chrono::steady_clock::now();
            system = hip.load_system(*program);
            const double ms_system = ms_since(t0);
            t0 = std::chrono::steady_clock::now();
            const Mapped prog_bytes(input);
            const ComputedWitness w = compute_one(hip, system, prog_bytes, arguments);
            const double ms_exec = ms_since(t0);
            proof = hip.prove(scheme, system, w, key, rng, &tm);
            tm.r1cs_upload = ms_system;
            tm.witness_to_assignment = ms_exec;
            printf("witness computed on the device from %zu arguments (%.3f ms)\n", arguments.size() / 32, ms_exec);
        } else {
            proof = check_first ? hip.prove(scheme, system, witness.data, witness.size, key, rng, &tm)
                                : hip.prove(scheme, *program, witness.data, witness.size, key, rng, &tm);
            if (check_first) tm.r1cs_upload = upload_ms;
        }
        t0 = std::chrono::steady_clock::now();
        {
            std::ofstream o(proof_path);
            if (!o) throw Error(ZKHIP_ERR_BAD_ARG, "cannot write " + proof_path);
            o << proof.to_json();
            o.close();
            if (!o) throw Error(ZKHIP_ERR_BAD_ARG, "error while writing " + proof_path);
        }
        const double ms_json = ms_since(t0);
        // --verify: the proof just written against the verification key at the head of the proving key, on the host CPU
        // (csrc/host/verify.cpp; ~40 ms on bn128) — a proof the pairing check refuses is an error, not an output
        double ms_verify = 0;
        if (self_check) {
            t0 = std::chrono::steady_clock::now();
            // only the head of the key file is read: the fixed points, the count, then that many G1 points
            const size_t fq = curve == ZKHIP_CURVE_BN128 ? 32 : 48, fixed = scheme == Scheme::GM17 ? 16 * fq : 14 * fq;
            std::vector<uint8_t> head(fixed + 8);
            std::ifstream kf(pk_path, std::ios::binary);
            if (!kf.read((char*)head.data(), (std::streamsize)head.size())) throw Error(ZKHIP_ERR_PARSE, "proving key too short for its verification key");
            uint64_t count;
            memcpy(&count, head.data() + fixed, 8);
            if (count > (1u << 24)) throw Error(ZKHIP_ERR_PARSE, "proving key: implausible number of public inputs");
            head.resize(fixed + 8 + count * 2 * fq);
            if (count && !kf.read((char*)head.data() + fixed + 8, (std::streamsize)(count * 2 * fq))) throw Error(ZKHIP_ERR_PARSE, "proving key too short for its verification key");
            const VerificationKey vk = VerificationKey::from_json(verification_key_json(scheme, curve, head.data(), head.size()));
            bool verified;
            if (device_verify) {
                const DeviceVerificationKey dvk = hip.load_verification_key(vk);
                verified = hip.verify_batch(dvk, {proof})[0];
            } else {
                verified = verify(vk, proof);
            }
            if (!verified) {
                remove(proof_path.c_str());
                throw Error(ZKHIP_ERR_UNSATISFIED, "the proof does not verify against the key of " + pk_path +
                                                       (check_first ? " (a key for another program: the witness satisfies this one)"
                                                                    : " (witness not satisfying the program, or a key for another program)"));
            }
            ms_verify = ms_since(t0);
            printf("verified against the verification key of %s\n", pk_path.c_str());
        }
        if (compact) printf("compact witness: %s\n", hip.last_witness_packed() ? "uploaded packed" : "dense, uploaded plain");
        if (device_witness)
            printf("device witness: %s\n", hip.last_witness_on_device() ? "read on the device" : compact ? "off (--compact-witness wins)" : "read on the host (the program has no plan)");
        printf("generate-proof (%s): wrote %s\n", scheme_s.c_str(), proof_path.c_str());
        const std::pair<int, int> where = cpu_and_node();
        if (timings)
            printf("timings {\"read_program_and_witness_ms\": %.3f, \"parse_program_ms\": %.3f, \"hip_init_ms\": %.3f, \"key_load_ms\": %.3f, "
                   "\"wait_for_host_side_ms\": %.3f, \"witness_to_assignment_ms\": %.3f, \"r1cs_upload_ms\": %.3f, \"prove_ms\": %.3f, "
                   "\"proof_json_ms\": %.3f, \"verify_ms\": %.3f, \"total_in_process_ms\": %.3f, \"key_source\": \"%s\", \"constraints\": %llu, "
                   "\"tables\": \"%s\", \"host_threads\": %u, \"cpu\": %d, \"numa_node\": %d}\n",
                   ms_read, ms_parse, ms_init, ms_key, ms_wait, tm.witness_to_assignment, tm.r1cs_upload, tm.prove, ms_json, ms_verify, ms_since(t_start),
                   key_source.c_str(), (unsigned long long)program->constraints(), resident_tables ? "every window multiple" : "none (one proof per process)",
                   std::thread::hardware_concurrency(), where.first, where.second);
        // one proof per process: the proof is on disk, so leave without tearing down 6 GiB of tables and the HIP runtime
        fflush(stdout);
        _exit(0);
    } catch (const Error& e) {
        fprintf(stderr, "zkhip-cli: %s\n", e.what());
        return 1;
    } catch (const std::exception& e) {
        fprintf(stderr, "zkhip-cli: %s\n", e.what());
        return 1;
    }
}
