// exec_levels.cpp — the level schedule of an instruction stream (csrc/xplan.h: xplan_schedule), alone — no device, no library.  Over
// hand-written and seeded random streams:
//   every instruction is scheduled exactly once, the levels partition the schedule, a level is sorted by (opcode, offset);
//   the three hazard rules hold for every pair of instructions that share a slot (read after write, write after read, write after
//   write: the later instruction of the stream sits strictly above the earlier);
//   levels are minimal: each instruction sits one above its binding constraint (level 1 without one) — computed here from the pairs,
//   not from the per-slot W / R the schedule keeps;
//   executing the schedule level by level, the items of each level in a seeded random order, gives the store and the verdict of
//   stream order — with the opcode bodies of csrc/wexec.cuh (wx_step, each lane's own words) over the host's field arithmetic.
// Built plain and under ASan + UBSan (tests/test_device_exec_wide.py).
//   g++ -O1 -g -std=c++17 -DZK_EMU -fsanitize=address,undefined -fno-sanitize-recover=undefined -I zokrates_amd/csrc tests/host/exec_levels.cpp
#include <cstdio>
#include <cstdlib>
#include <random>
#include <set>

#include "wexec.cuh"

using namespace zk;
typedef Fe<Bn254Fr> Fr;

static int bad = 0;
static void expect(bool ok, const char* what, long long a = -1, long long b = -1) {
    if (!ok) { printf("FAILED %s (%lld, %lld)\n", what, a, b); ++bad; }
}

struct Code {
    std::vector<uint32_t> code, pool;
    uint32_t slots = 0, n_args = 0;
    std::vector<uint8_t> args;
};
struct Instr { uint32_t at; std::set<uint32_t> reads, writes; };

static std::vector<Instr> instructions(const Code& s) {
    std::vector<Instr> out;
    for (uint32_t pc = 0;;) {
        Instr in;
        in.at = pc;
        const uint32_t next = xplan_walk(s.code.data(), pc, [&](uint32_t x) { in.reads.insert(x); }, [&](uint32_t x) { in.writes.insert(x); });
        if (next == pc) break;
        out.push_back(in);
        pc = next;
    }
    return out;
}
static bool shares(const std::set<uint32_t>& a, const std::set<uint32_t>& b) {
    for (uint32_t x : a) if (b.count(x)) return true;
    return false;
}
// does the later instruction j have to sit above the earlier i?
static bool ordered(const Instr& i, const Instr& j) { return shares(i.writes, j.reads) || shares(i.reads, j.writes) || shares(i.writes, j.writes); }

// the store (and the verdict) after the instructions at `order`
static void execute(const Code& s, const std::vector<uint32_t>& order, std::vector<Fr>& store, uint32_t& verdict) {
    store.assign(s.slots, Fr::zero());
    store[0] = Fr::one();
    verdict = WX_RAN_THROUGH;
    for (uint32_t at : order) {
        uint32_t pc = at + 1, failed = WX_RAN_THROUGH;
        const bool known = wx_step<Fr, false>(s.code[at], s.code.data(), pc, s.pool.data(), s.args.data(), s.n_args, 0, store.data(), 1, Fr::one(), failed);
        expect(known, "an opcode the kernel knows", at);
        verdict = std::min(verdict, failed);
    }
}

static void check(const Code& s, const char* name, uint32_t seed, const std::vector<uint32_t>* want_levels = nullptr) {
    const std::vector<Instr> ins = instructions(s);
    expect(!ins.empty() && s.code[ins.back().at] != XOP_END && s.code.back() == XOP_END, "the stream is walked to its end");
    std::vector<uint32_t> sched, level_start;
    xplan_schedule(s.code, s.slots, sched, level_start);
    // once each
    expect(sched.size() == ins.size(), "as many entries as instructions", (long long)sched.size(), (long long)ins.size());
    std::vector<uint32_t> sorted = sched, offsets;
    std::sort(sorted.begin(), sorted.end());
    for (const Instr& in : ins) offsets.push_back(in.at);
    expect(sorted == offsets, "every instruction is scheduled exactly once");
    expect(!level_start.empty() && level_start[0] == 0 && level_start.back() == sched.size() && std::is_sorted(level_start.begin(), level_start.end()),
           "the levels partition the schedule");
    if (bad) return;
    std::vector<uint32_t> level_of_offset(s.code.size(), 0);
    for (size_t L = 0; L + 1 < level_start.size(); ++L) {
        expect(level_start[L] < level_start[L + 1], "no level is empty", (long long)L);
        for (uint32_t k = level_start[L]; k < level_start[L + 1]; ++k) {
            level_of_offset[sched[k]] = (uint32_t)L + 1;
            if (k > level_start[L]) {
                const uint32_t a = sched[k - 1], b = sched[k];
                expect(s.code[a] < s.code[b] || (s.code[a] == s.code[b] && a < b), "a level is sorted by opcode, then offset", a, b);
            }
        }
    }
    // the hazard rules, pair by pair, and minimality
    for (size_t j = 0; j < ins.size(); ++j) {
        const uint32_t Lj = level_of_offset[ins[j].at];
        uint32_t binding = 0;
        for (size_t i = 0; i < j; ++i) {
            if (!ordered(ins[i], ins[j])) continue;
            const uint32_t Li = level_of_offset[ins[i].at];
            expect(Lj > Li, "the later of two instructions that share a slot sits above the earlier", ins[i].at, ins[j].at);
            binding = std::max(binding, Li);
        }
        expect(Lj == binding + 1, "an instruction sits one above its binding constraint", ins[j].at, Lj);
        if (want_levels) expect((*want_levels)[j] == Lj, name, (long long)j, Lj);
    }
    // the same store in stream order and level by level, each level shuffled
    std::vector<Fr> a, b;
    uint32_t va, vb;
    execute(s, offsets, a, va);
    std::mt19937 rnd(seed);
    for (int round = 0; round < 3; ++round) {
        std::vector<uint32_t> order = sched;
        for (size_t L = 0; L + 1 < level_start.size(); ++L) std::shuffle(order.begin() + level_start[L], order.begin() + level_start[L + 1], rnd);
        execute(s, order, b, vb);
        bool equal = va == vb;
        for (uint32_t k = 0; k < s.slots; ++k) equal = equal && a[k].equals(b[k]);
        expect(equal, "a shuffled level-by-level execution leaves the store and the verdict of stream order", seed, round);
    }
}

// ---- writing streams
struct Writer {
    Code s;
    std::mt19937 rnd;
    std::vector<uint32_t> written{0};      // slots that hold a value
    uint32_t statement = 0;
    explicit Writer(uint32_t seed, uint32_t slots, uint32_t n_args) : rnd(seed) {
        s.slots = slots;
        s.n_args = n_args;
        const uint64_t coeffs[] = {1, 0, 2, 5, 0x123456789abcdefull};
        for (int k = 0; k < 5; ++k) {
            Fr c = Fr::zero();
            c.v[0] = (uint32_t)coeffs[k]; c.v[1] = (uint32_t)(coeffs[k] >> 32);
            Fr m = k == 1 ? fe_neg(Fr::one()) : fe_to_mont(c);
            s.pool.insert(s.pool.end(), m.v, m.v + 8);
        }
        s.args.assign((size_t)n_args * 32, 0);
        for (uint32_t k = 0; k < n_args; ++k)
            for (int b = 0; b < 12; ++b) s.args[k * 32 + b] = (uint8_t)(k < 2 ? k : rnd());      // arguments 0 and 1, then 96-bit integers
    }
    uint32_t pick(uint32_t n) { return (uint32_t)(rnd() % n); }
    void lc(const std::vector<std::pair<uint32_t, uint32_t>>& terms) {
        s.code.push_back((uint32_t)terms.size());
        for (auto& t : terms) { s.code.push_back(t.first); s.code.push_back(t.second); }
    }
    void random_lc() {
        std::vector<std::pair<uint32_t, uint32_t>> t(pick(4));
        for (auto& x : t) x = {written[pick((uint32_t)written.size())], pick(5)};
        lc(t);
    }
    void quad() { random_lc(); random_lc(); }
    uint32_t out() { return 1 + pick(s.slots - 1); }      // any slot but ~one: fresh, or one that holds a value (an overwrite)
    void mark(uint32_t slot) { written.push_back(slot); }
    void arg(uint32_t k, uint32_t slot) { s.code.insert(s.code.end(), {XOP_ARG, k, slot}); mark(slot); }
    void random_instruction() {
        const uint32_t kind = pick(12);
        if (kind < 4) { const uint32_t o = out(); s.code.insert(s.code.end(), {XOP_DEFINE, o}); quad(); mark(o); }
        else if (kind < 6) { s.code.insert(s.code.end(), {XOP_CHECK, statement}); quad(); random_lc(); }
        else if (kind == 6) { const uint32_t a = out(), b = out(); s.code.insert(s.code.end(), {XOP_CONDEQ, a, b}); quad(); mark(a); mark(b); }
        else if (kind == 7) {
            const uint32_t n = pick(8) == 0 ? 300 : 1 + pick(6);
            s.code.insert(s.code.end(), {XOP_BITS, n});
            quad();
            for (uint32_t k = 0; k < n; ++k) { const uint32_t o = out(); s.code.push_back(o); mark(o); }
        }
        else if (kind == 8) { const uint32_t o = out(); s.code.insert(s.code.end(), {(uint32_t)(XOP_DIV + pick(3)), o}); quad(); quad(); mark(o); }
        else if (kind == 9) { const uint32_t o = out(); s.code.insert(s.code.end(), {(uint32_t)(XOP_SHA3 + pick(2)), o}); quad(); quad(); quad(); mark(o); }
        else if (kind == 10) { const uint32_t a = out(), b = out(); s.code.insert(s.code.end(), {XOP_EDIV, a, b}); quad(); quad(); mark(a); mark(b); }
        else if (s.n_args) arg(pick(s.n_args), out());      // (a repeated parameter: an argument stored again)
        ++statement;
    }
    Code end() { s.code.push_back(XOP_END); return s; }
};

int main() {
    const uint32_t ONE_ = XCOEFF_ONE;
    {   // write after read: x defined, y = x x, a ConditionEq overwrites x, z = x 1
        Writer w(1, 8, 1);
        w.arg(0, 1);
        w.s.code.insert(w.s.code.end(), {XOP_DEFINE, 2}); w.lc({{1, ONE_}}); w.lc({{1, ONE_}, {0, 3}});      // x = a (a + 5)        2
        w.s.code.insert(w.s.code.end(), {XOP_DEFINE, 3}); w.lc({{2, ONE_}}); w.lc({{2, ONE_}});              // y = x x              3
        w.s.code.insert(w.s.code.end(), {XOP_CONDEQ, 2, 4}); w.lc({{1, ONE_}}); w.lc({{0, ONE_}});           // x := (a != 0)        4
        w.s.code.insert(w.s.code.end(), {XOP_DEFINE, 5}); w.lc({{2, ONE_}}); w.lc({{0, ONE_}});              // z = x                5
        const std::vector<uint32_t> want = {1, 2, 3, 4, 5};
        check(w.end(), "write after read: the levels counted by hand", 11, &want);
    }
    {   // write after write with no reader between; a directive whose output is its input; a check; independent defines
        Writer w(2, 10, 2);
        w.arg(0, 1); w.arg(1, 2);                                                                            //                      1 1
        w.s.code.insert(w.s.code.end(), {XOP_DIV, 3}); w.lc({{1, ONE_}}); w.lc({{0, ONE_}}); w.lc({{2, ONE_}}); w.lc({{0, ONE_}});      // v = a / b       2
        w.s.code.insert(w.s.code.end(), {XOP_CONDEQ, 3, 4}); w.lc({{2, ONE_}}); w.lc({{0, ONE_}});           // v := (b != 0)        3
        w.s.code.insert(w.s.code.end(), {XOP_CONDEQ, 1, 5}); w.lc({{1, ONE_}}); w.lc({{2, ONE_}});           // a := (a b != 0): above a's reader at 2     3
        w.s.code.insert(w.s.code.end(), {XOP_CHECK, 7}); w.lc({{1, ONE_}}); w.lc({{1, ONE_}}); w.lc({{1, ONE_}});      // a a == a    4
        w.s.code.insert(w.s.code.end(), {XOP_DEFINE, 6}); w.lc({{2, ONE_}}); w.lc({{2, 3}});                 // b (5 b)              2
        w.s.code.insert(w.s.code.end(), {XOP_ARG, 1, 2});                                                    // b again: above every reader of b (levels 2, 3 read it: 2, 3, 2)   4
        const std::vector<uint32_t> want = {1, 1, 2, 3, 3, 4, 2, 4};
        check(w.end(), "write after write, own input, repeated parameter: the levels counted by hand", 12, &want);
    }
    {   // nothing but arguments, and an empty program
        Writer w(3, 4, 3);
        w.arg(0, 1); w.arg(1, 2); w.arg(2, 3);
        const std::vector<uint32_t> want = {1, 1, 1};
        check(w.end(), "arguments alone are one level", 13, &want);
        Code empty;
        empty.slots = 1;
        empty.code.push_back(XOP_END);
        std::vector<uint32_t> sched, level_start;
        xplan_schedule(empty.code, 1, sched, level_start);
        expect(sched.empty() && level_start.size() == 1 && level_start[0] == 0, "an empty stream has no level");
    }
    // seeded random streams: few slots (every hazard, often), many slots (wide levels)
    for (uint32_t seed = 0; seed < 60; ++seed) {
        const uint32_t slots = seed % 3 == 0 ? 6 : seed % 3 == 1 ? 24 : 400, n_args = 1 + seed % 4;
        Writer w(0x5EED00 + seed, slots, n_args);
        for (uint32_t k = 0; k < n_args; ++k) w.arg(k, 1 + k % (slots - 1));
        const uint32_t count = seed % 3 == 2 ? 250 : 60;
        for (uint32_t k = 0; k < count; ++k) w.random_instruction();
        check(w.end(), "a random stream", 100 + seed);
    }
    printf("%d failures\n", bad);
    return bad ? 1 : 0;
}
