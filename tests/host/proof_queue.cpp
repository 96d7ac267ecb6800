// TEST PROGRAM for the proof queue of the compiled host side (include/zkhip_backend.hpp: Hip::open_queue, Queue::submit / collect): one
// system and its two keys resident, three witnesses.  For each scheme and key state (as loaded, bound), in one witness form (plain or
// compact, alternating, so that each form meets each scheme and each key state): seven proofs through Hip::prove from one StdRng seed, then the same seven through a Queue from the same seed in the steady-state
// order (submit until full, then collect one per submit) — the same proof.json text, proof for proof.  Besides: the Hip refuses to
// prove beside its open queue and proves again once the queue is closed with proofs uncollected; a full queue refuses a submit
// without touching the RNG.
// usage: proof_queue <out> <proving.key (g16)> <proving.key (gm17)> <witness> <witness> <witness> [g16]      ("g16": that scheme only)
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
    fprintf(stderr, "proof_queue: FAILED %s (%d, %d)\n", what, a, b);
}

int main(int argc, char** argv) {
    if (argc != 7 && argc != 8) return 2;
    const int schemes = argc == 8 && std::string(argv[7]) == "g16" ? 1 : 2;
    try {
        const std::vector<uint8_t> out = slurp(argv[1]);
        const std::vector<uint8_t> keys[2] = {slurp(argv[2]), slurp(argv[3])};
        const std::vector<uint8_t> wit[3] = {slurp(argv[4]), slurp(argv[5]), slurp(argv[6])};
        const int count = 7;
        Hip hip(0);
        Program prog(out.data(), out.size());
        System sys = hip.load_system(prog);
        for (int sc = 0; sc < schemes; ++sc) {
            const Scheme scheme = sc ? Scheme::GM17 : Scheme::G16;
            Key key = hip.load_proving_key(scheme, prog.curve(), keys[sc].data(), keys[sc].size());
            for (int bound = 0; bound < 2; ++bound) {
                if (bound) expect(hip.bind(key, sys) && hip.is_bound(key, sys), "bind", sc);
                // (each witness form with each key state, over the two schemes: G16 plain / bound compact, GM17 compact / bound plain)
                for (int compact = (sc + bound) & 1; compact <= ((sc + bound) & 1); ++compact) {
                    hip.set_compact_witness(compact != 0);
                    StdRng rng = get_rng_from_entropy("one witness at a time");
                    std::vector<std::string> want;
                    bool packed = false;
                    for (int i = 0; i < count; ++i) {
                        want.push_back(hip.prove(scheme, sys, wit[i % 3].data(), wit[i % 3].size(), key, rng).to_json());
                        packed = hip.last_witness_packed();
                    }
                    expect(want[0] != want[3], "fresh randomness per proof", sc, compact);
                    StdRng rng2 = get_rng_from_entropy("one witness at a time");
                    Queue q = hip.open_queue(scheme, sys, key);
                    expect(q.capacity() >= 1 && q.in_flight() == 0 && !q.ready(), "a fresh queue", sc, compact);
                    int got = 0;
                    for (int i = 0; i < count; ++i) {
                        if (q.full()) {
                            uint64_t t = ~0ull;
                            expect(q.collect(&t).to_json() == want[got] && t == (uint64_t)got, "steady-state proof", sc * 100 + bound * 10 + compact, got);
                            ++got;
                        }
                        expect(q.submit(wit[i % 3].data(), wit[i % 3].size(), rng2) == (uint64_t)i, "ticket", sc, i);
                        expect(q.last_witness_packed() == packed, "the compact rule of Hip::prove", sc, compact);
                    }
                    // full: a submit is refused before it draws from the RNG; the Hip proves nothing beside its queue
                    if (q.full()) {
                        StdRng a = get_rng_from_entropy("untouched"), b = get_rng_from_entropy("untouched");
                        try {
                            q.submit(wit[0].data(), wit[0].size(), a);
                            expect(false, "a full queue accepted a submit");
                        } catch (const Error& e) {
                            expect(e.code == ZKHIP_ERR_BUSY, "ZKHIP_ERR_BUSY", e.code);
                        }
                        expect(a.next_u64() == b.next_u64(), "a refused submit drew from the RNG");
                    }
                    try {
                        StdRng a = get_rng_from_entropy("beside");
                        hip.prove(scheme, sys, wit[0].data(), wit[0].size(), key, a);
                        expect(false, "Hip::prove beside an open queue");
                    } catch (const Error& e) {
                        expect(e.code == ZKHIP_ERR_BAD_ARG && std::string(e.what()).find("proof queue") != std::string::npos, "the refusal names the queue", e.code);
                    }
                    while (q.in_flight()) {
                        expect(q.collect().to_json() == want[got], "drained proof", sc * 100 + bound * 10 + compact, got);
                        ++got;
                    }
                    expect(got == count, "every proof collected", got, count);
                    try {
                        q.collect();
                        expect(false, "collect on an empty queue");
                    } catch (const Error& e) {
                        expect(e.code == ZKHIP_ERR_BAD_ARG, "empty: ZKHIP_ERR_BAD_ARG", e.code);
                    }
                    // closed with two proofs uncollected: the Hip is an ordinary prover again
                    StdRng rng3 = get_rng_from_entropy("one witness at a time");
                    q.submit(wit[0].data(), wit[0].size(), rng3);
                    q.submit(wit[1].data(), wit[1].size(), rng3);
                    q.close();
                    StdRng rng4 = get_rng_from_entropy("one witness at a time");
                    expect(hip.prove(scheme, sys, wit[0].data(), wit[0].size(), key, rng4).to_json() == want[0], "prove after close", sc, compact);
                }
            }
        }
        hip.set_compact_witness(false);
        if (failures) return 1;
        printf("proof queue host checks OK\n");
        return 0;
    } catch (const std::exception& e) {
        fprintf(stderr, "proof_queue: %s\n", e.what());
        return 1;
    }
}
