// TEST PROGRAM for witness files read on the device, from the compiled host side (include/zkhip_backend.hpp: Hip::set_device_witness,
// last_witness_on_device, Queue::last_witness_on_device): one system and its key resident, three witnesses.  Seven proofs through
// Hip::prove and seven through a Queue with the setting ON are, from equal StdRng seeds, the proof.json text of the same calls with
// the setting off — proofs and inputs.  Besides: set_compact_witness wins when both are set; a program the plan refuses (a repeated
// parameter) falls back to the host reader and says so; the setting is read when a queue is opened.
// usage: witness_queue <out> <proving.key (g16)> <witness> <witness> <witness> <out with a repeated parameter>
#include <cstdio>
#include <fstream>
#include <iterator>

#include "../../include/zkhip_backend.hpp"

using namespace zokrates_hip;

static std::vector<uint8_t> slurp(const char* path) {
    std::ifstream f(path, std::ios::binary);
    return std::vector<uint8_t>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}
static int failures = 0;
static void expect(bool ok, const char* what, int a = -1, int b = -1) {
    if (ok) return;
    ++failures;
    fprintf(stderr, "witness_queue: FAILED %s (%d, %d)\n", what, a, b);
}

int main(int argc, char** argv) {
    if (argc != 7) return 2;
    try {
        const std::vector<uint8_t> out = slurp(argv[1]), key_bytes = slurp(argv[2]), repeated = slurp(argv[6]);
        const std::vector<uint8_t> wit[3] = {slurp(argv[3]), slurp(argv[4]), slurp(argv[5])};
        const int count = 7;
        const Scheme scheme = Scheme::G16;
        Hip hip(0);
        Program prog(out.data(), out.size());
        System sys = hip.load_system(prog);
        Key key = hip.load_proving_key(scheme, prog.curve(), key_bytes.data(), key_bytes.size());
        expect(!hip.set_device_witness(false) && !hip.last_witness_on_device(), "off by default");
        for (int bound = 0; bound < 2; ++bound) {
            if (bound) expect(hip.bind(key, sys) && hip.is_bound(key, sys), "bind");
            // the host reader's proofs
            hip.set_device_witness(false);
            StdRng rng = get_rng_from_entropy("files to proofs");
            std::vector<std::string> want;
            for (int i = 0; i < count; ++i) {
                want.push_back(hip.prove(scheme, sys, wit[i % 3].data(), wit[i % 3].size(), key, rng).to_json());
                expect(!hip.last_witness_on_device(), "host reader", i);
            }
            expect(want[0] != want[3] && want[0].find("\"inputs\"") != std::string::npos, "fresh randomness per proof, inputs in the text");
            // Hip::prove with the setting on
            expect(!hip.set_device_witness(true), "the previous setting");
            StdRng rng1 = get_rng_from_entropy("files to proofs");
            for (int i = 0; i < count; ++i) {
                expect(hip.prove(scheme, sys, wit[i % 3].data(), wit[i % 3].size(), key, rng1).to_json() == want[i], "Hip::prove from the device route", bound, i);
                expect(hip.last_witness_on_device() && !hip.last_witness_packed(), "device route", i);
            }
            // a Queue opened with the setting on, in the steady-state order
            StdRng rng2 = get_rng_from_entropy("files to proofs");
            Queue q = hip.open_queue(scheme, sys, key);
            int got = 0;
            for (int i = 0; i < count; ++i) {
                if (q.full()) {
                    uint64_t t = ~0ull;
                    expect(q.collect(&t).to_json() == want[got] && t == (uint64_t)got, "steady-state proof", bound, got);
                    ++got;
                }
                expect(q.submit(wit[i % 3].data(), wit[i % 3].size(), rng2) == (uint64_t)i, "ticket", i);
                expect(q.last_witness_on_device() && !q.last_witness_packed(), "the queue's device route", i);
            }
            while (q.in_flight()) {
                expect(q.collect().to_json() == want[got], "drained proof", bound, got);
                ++got;
            }
            expect(got == count, "every proof collected", got, count);
            q.close();
            // the setting is read when the queue is opened: one opened with it off keeps the host reader
            hip.set_device_witness(false);
            StdRng rng3 = get_rng_from_entropy("files to proofs");
            Queue q2 = hip.open_queue(scheme, sys, key);
            hip.set_device_witness(true);
            q2.submit(wit[0].data(), wit[0].size(), rng3);
            expect(!q2.last_witness_on_device(), "a queue opened with the setting off");
            expect(q2.collect().to_json() == want[0], "its proof");
            q2.close();
            // compact wins if both are set
            hip.set_compact_witness(true);
            StdRng rng4 = get_rng_from_entropy("files to proofs");
            expect(hip.prove(scheme, sys, wit[0].data(), wit[0].size(), key, rng4).to_json() == want[0], "both set: the same proof");
            expect(!hip.last_witness_on_device(), "both set: compact wins");
            Queue q3 = hip.open_queue(scheme, sys, key);
            q3.submit(wit[1].data(), wit[1].size(), rng4);
            expect(!q3.last_witness_on_device(), "both set, queue: compact wins");
            expect(q3.collect().to_json() == want[1], "both set, queue: the same proof");
            q3.close();
            hip.set_compact_witness(false);
            // a defect of the file is the library's error: a truncated file, from both routes
            for (int device = 0; device < 2; ++device) {
                hip.set_device_witness(device != 0);
                try {
                    StdRng a = get_rng_from_entropy("x");
                    hip.prove(scheme, sys, wit[0].data(), wit[0].size() - 1, key, a);
                    expect(false, "a truncated file was accepted", device);
                } catch (const Error& e) {
                    expect(e.code == ZKHIP_ERR_PARSE, "ZKHIP_ERR_PARSE", e.code, device);
                }
            }
        }
        // a program the plan refuses keeps the host reader, and says so
        {
            Program prog2(repeated.data(), repeated.size());
            System sys2 = hip.load_system(prog2);
            hip.set_device_witness(true);
            StdRng a = get_rng_from_entropy("x");
            try {
                hip.prove(scheme, sys2, wit[0].data(), wit[0].size(), key, a);
                expect(false, "a repeated parameter was accepted");
            } catch (const Error& e) {      // the HOST reader's refusal: the route that was taken
                expect(e.code == ZKHIP_ERR_UNSATISFIED && std::string(e.what()).find("consumed twice") != std::string::npos, "the host reader's message", e.code);
            }
            expect(!hip.last_witness_on_device(), "a refused program falls back to the host reader");
        }
        hip.set_device_witness(false);
        if (failures) return 1;
        printf("witness queue host checks OK\n");
        return 0;
    } catch (const std::exception& e) {
        fprintf(stderr, "witness_queue: %s\n", e.what());
        return 1;
    }
}
