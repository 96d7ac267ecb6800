// xplan.h — the host side of witnesses computed on the device (include/zkhip.h "witnesses computed on the device"): a ZoKrates program's
// statements compiled, once, into the instruction stream that wexec.cuh's k_exec_program runs for every instance of a batch.
//
//   Interpreter::execute      /root/reference/zokrates_interpreter/src/lib.rs:30-138 (the walk), :167-352 (execute_solver),
//                             :366-378 (evaluate_lin, evaluate_quad)
//   LinComb::is_assignee      /root/reference/zokrates_ast/src/ir/expression.rs:218-222
//   Solver::get_signature     /root/reference/zokrates_ast/src/common/solvers.rs:52-69
//   Witness (BTreeMap order)  /root/reference/zokrates_ast/src/ir/witness.rs:44-53, common/flat/variable.rs:10-13
//
// An ir::Prog is a straight-line list and no control flow depends on a value: which constraint DEFINES its variable and which one CHECKS
// is decided by the program alone (`defined` below is what `witness.0.contains_key` answers at that point, whatever the arguments), so
// every instance of a batch executes the same instruction at the same time.  The statements section of the same `out` bytes that
// zkhip_prog_parse read is walked a second time, with the combinations RAW — no duplicates merged, no zero coefficients dropped:
// is_assignee looks at the raw LinComb, which the R1CS inside zkhip_prog no longer has.
//
// The plan also holds the stream's LEVEL SCHEDULE (xplan_schedule below): which instructions depend on which is a property of the
// stream alone, computed here once, for the level-scheduled route of wexec.cuh (k_exec_level, k_exec_levels_run).
//
// Pure host code over ingest.h's zkhip_prog and field.cuh (tests/host/exec_plan.cpp and exec_levels.cpp compile it alone); the kernels are in wexec.cuh,
// the resident plan and the entry points in core.cuh / zkhip_api.hip.
#pragma once
#include <algorithm>
#include <array>
#include <cstring>
#include <map>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/zkhip.h"
#include "field.cuh"
#include "ingest.h"
#include "wplan.h"

namespace zk {

// ---- the instruction stream: 32-bit words.  LC = n, then n x (slot, coefficient);  Q = LC left, LC right (a QuadComb)
//   XOP_ARG     k, slot                      argument k of the instance, converted as it enters
//   XOP_DEFINE  slot, Q                      slot = left * right
//   XOP_CHECK   statement, Q, LC             left * right == lin, else the instance fails at `statement`
//   XOP_CONDEQ  out0, out1, Q                [0, 1] for zero, else [1, 1/x]
//   XOP_BITS    n, Q, n x out                out i = bit n - 1 - i of the canonical integer
//   XOP_DIV / XOP_XOR / XOP_OR   out, Q, Q
//   XOP_SHA3 / XOP_SHACH         out, Q, Q, Q
//   XOP_EDIV    q, r, Q, Q                   integer division of the canonical values
//   XOP_END
// (a directive's inputs are all evaluated before its first output is stored: an output may be a variable an input reads)
// coefficient 0 is the value 1 and coefficient 1 the value -1 (an addition, a subtraction: most terms of a compiled program); the
// others index the pool (eight words each, Montgomery form)
enum XOp : uint32_t { XOP_END = 0, XOP_ARG, XOP_DEFINE, XOP_CHECK, XOP_CONDEQ, XOP_BITS, XOP_DIV, XOP_XOR, XOP_OR, XOP_SHA3, XOP_SHACH, XOP_EDIV };
static constexpr uint32_t XCOEFF_ONE = 0, XCOEFF_MINUS_ONE = 1;
static constexpr uint64_t XPLAN_MAX_BITS = 1 << 16;      // outputs of one Bits directive
static constexpr uint32_t XPLAN_NO_ROW = 0xffffffffu;

// what a plan knows on the host
struct XPlanHost {
    int curve = 0;
    uint64_t n = 0, l = 0, w = 0;
    uint64_t n_args = 0, n_statements = 0, n_defines = 0, n_checks = 0, n_directives = 0, n_extra = 0;
    uint64_t slots = 0;                    // l + w + n_extra: column j of the R1CS is slot j, a variable without a column sits above
    std::vector<uint32_t> code;
    std::vector<uint32_t> pool;            // 8 words per coefficient; [0] = 1, [1] = -1
    std::vector<int64_t> file_ids;         // ascending signed ids of every variable the interpreter's Witness holds
    std::vector<uint32_t> file_slots;      // their slots
    std::vector<uint32_t> input_cols;      // public arguments in argument order, then ~out_0 .. ~out_{R-1} (as WPlanTables)
    std::vector<uint32_t> row_of;          // R1CS row of statement k (XPLAN_NO_ROW: not a constraint)
    // the level schedule (xplan_schedule below): the word offset of every instruction by (level, opcode, offset), and where each
    // level begins in it (levels + 1 entries; level L of the text is level_start[L - 1] .. level_start[L])
    std::vector<uint32_t> sched;
    std::vector<uint32_t> level_start;
    uint64_t store_bytes_per_instance() const { return slots * 32; }
    uint64_t file_bytes() const { return 8 + 40 * (uint64_t)file_ids.size(); }
    void dims(uint64_t out[8]) const {
        out[0] = n_args; out[1] = n_statements; out[2] = n_defines; out[3] = n_checks; out[4] = n_directives; out[5] = file_ids.size();
        out[6] = n_extra; out[7] = store_bytes_per_instance();
    }
    void levels(uint64_t out[4]) const {
        const uint64_t nl = level_start.empty() ? 0 : level_start.size() - 1;
        out[0] = nl; out[1] = 0; out[2] = sched.size(); out[3] = 0;
        for (uint64_t k = 0; k < nl; ++k) {
            const uint64_t width = level_start[k + 1] - level_start[k];
            out[1] = std::max(out[1], width);
            out[3] += width < 64;
        }
    }
};

// ---- the level schedule: which instructions of a stream may run side by side
// One instruction of the stream at word `pc`: read(slot) for every slot a combination names, THEN write(slot) for every slot it
// stores (an instruction evaluates all its inputs before its first store).  Returns the offset of the next instruction; XOP_END and
// a word that is no opcode return `pc` itself.
template <class Read, class Write>
inline uint32_t xplan_walk(const uint32_t* code, uint32_t pc, Read&& read, Write&& write) {
    const uint32_t op = code[pc];
    uint32_t at = pc + 1;
    auto lcs = [&](int count) {
        for (int k = 0; k < count; ++k) {
            const uint32_t n = code[at++];
            for (uint32_t t = 0; t < n; ++t, at += 2) read(code[at]);
        }
    };
    switch (op) {
        case XOP_ARG: write(code[at + 1]); return at + 2;
        case XOP_DEFINE: { const uint32_t o = code[at++]; lcs(2); write(o); return at; }
        case XOP_CHECK: ++at; lcs(3); return at;
        case XOP_CONDEQ: { const uint32_t o0 = code[at], o1 = code[at + 1]; at += 2; lcs(2); write(o0); write(o1); return at; }
        case XOP_BITS: { const uint32_t n = code[at++]; lcs(2); for (uint32_t k = 0; k < n; ++k) write(code[at + k]); return at + n; }
        case XOP_DIV: case XOP_XOR: case XOP_OR: { const uint32_t o = code[at++]; lcs(4); write(o); return at; }
        case XOP_SHA3: case XOP_SHACH: { const uint32_t o = code[at++]; lcs(6); write(o); return at; }
        case XOP_EDIV: { const uint32_t o0 = code[at], o1 = code[at + 1]; at += 2; lcs(4); write(o0); write(o1); return at; }
        default: return pc;
    }
}
// Levels of a stream over `slots` slots.  Per slot W, the level of the last write (slot 0, ~one, counts as written at level 0, before
// the first level runs) and R, the highest level that read the current value (0 after a write).  An instruction sits at the smallest
// L >= 1 above W of every slot it reads (read after write) and above W and R of every slot it writes (write after write, write after
// read: a directive's output may overwrite a defined variable, a repeated parameter writes twice — both land strictly after every
// reader of the old value).  The instructions of one level run in no order.  `sched` is sorted by level, then opcode, then offset,
// so that neighbouring work-items mostly run one arm of the kernel's switch.
inline void xplan_schedule(const std::vector<uint32_t>& code, uint64_t slots, std::vector<uint32_t>& sched, std::vector<uint32_t>& level_start) {
    std::vector<uint32_t> W(slots, 0), R(slots, 0), level_of;
    sched.clear();
    uint32_t top = 0;
    for (uint32_t pc = 0;;) {
        uint32_t L = 0;
        const uint32_t next = xplan_walk(code.data(), pc, [&](uint32_t s) { L = std::max(L, W[s]); },
                                         [&](uint32_t s) { L = std::max(L, std::max(W[s], R[s])); });
        if (next == pc) break;
        ++L;
        xplan_walk(code.data(), pc, [&](uint32_t s) { R[s] = std::max(R[s], L); }, [&](uint32_t s) { W[s] = L; R[s] = 0; });
        sched.push_back(pc);
        level_of.push_back(L);
        top = std::max(top, L);
        pc = next;
    }
    std::vector<uint32_t> idx(sched.size());
    for (uint32_t k = 0; k < idx.size(); ++k) idx[k] = k;
    std::sort(idx.begin(), idx.end(), [&](uint32_t a, uint32_t b) {
        if (level_of[a] != level_of[b]) return level_of[a] < level_of[b];
        if (code[sched[a]] != code[sched[b]]) return code[sched[a]] < code[sched[b]];
        return sched[a] < sched[b];
    });
    level_start.assign((size_t)top + 1, 0);
    for (uint32_t L : level_of) ++level_start[L];      // [L] = width of level L; [0] = 0
    for (uint32_t L = 1; L <= top; ++L) level_start[L] += level_start[L - 1];      // [L] = end of level L = start of level L + 1
    std::vector<uint32_t> sorted(sched.size());
    for (uint32_t k = 0; k < idx.size(); ++k) sorted[k] = sched[idx[k]];
    sched.swap(sorted);
}

namespace xplan_detail {

[[noreturn]] inline void fail(int32_t code, const std::string& msg) { throw IngestError{code, msg}; }

// a pull reader of the CBOR [UPSTREAM] serde_cbor 0.11.2 writes for the derived shapes (ingest.hip holds the same subset for the
// constraint reader, inside its translation unit)
struct XCbor {
    const uint8_t *p, *e;
    struct Head { int major; uint64_t arg; bool indef; };
    static constexpr uint64_t INDEF = ~(uint64_t)0;
    const uint8_t* take(uint64_t n) {
        if ((uint64_t)(e - p) < n) fail(ZKHIP_ERR_PARSE, "program file truncated inside a CBOR item");
        const uint8_t* r = p;
        p += n;
        return r;
    }
    Head head() {
        const uint8_t b = *take(1);
        Head h{b >> 5, 0, false};
        const int ai = b & 31;
        if (ai < 24) h.arg = ai;
        else if (ai <= 27) {
            const int nb = 1 << (ai - 24);
            const uint8_t* q = take(nb);
            for (int i = 0; i < nb; ++i) h.arg = (h.arg << 8) | q[i];
        } else if (ai == 31) h.indef = true;
        else fail(ZKHIP_ERR_PARSE, "malformed CBOR (reserved additional information)");
        return h;
    }
    bool is_break() const { return p < e && *p == 0xff; }
    void skip(int depth = 0) {
        if (depth > 64) fail(ZKHIP_ERR_PARSE, "CBOR nesting too deep");
        const Head h = head();
        if (h.major <= 1) return;
        if (h.major <= 3) {
            if (!h.indef) { take(h.arg); return; }
            while (!is_break()) skip(depth + 1);
            take(1);
        } else if (h.major <= 5) {
            if (!h.indef) {
                // (every item takes a byte at least: a count beyond what is left is a truncated file, not hours of looping)
                if (h.arg > (uint64_t)(e - p)) fail(ZKHIP_ERR_PARSE, "program file truncated inside a CBOR item");
                for (uint64_t i = 0; i < h.arg * (h.major == 5 ? 2 : 1); ++i) skip(depth + 1);
                return;
            }
            while (!is_break()) skip(depth + 1);
            take(1);
        } else if (h.major == 6) {
            skip(depth + 1);
        } else if (h.indef) {
            fail(ZKHIP_ERR_PARSE, "malformed CBOR (unexpected break)");
        }
    }
    uint64_t enter(int major, const char* what) {
        const Head h = head();
        if (h.major != major) fail(ZKHIP_ERR_PARSE, std::string("unexpected CBOR type where ") + what + " was expected");
        if (!h.indef && h.arg > (uint64_t)(e - p)) fail(ZKHIP_ERR_PARSE, "program file truncated inside a CBOR item");
        return h.indef ? INDEF : h.arg;
    }
    bool more(uint64_t& remaining) {
        if (remaining == INDEF) {
            if (is_break()) { take(1); return false; }
            if (p >= e) fail(ZKHIP_ERR_PARSE, "program file truncated inside a CBOR item");
            return true;
        }
        if (remaining == 0) return false;
        --remaining;
        return true;
    }
    std::string text(const char* what) {
        const Head h = head();
        if (h.major != 3 || h.indef) fail(ZKHIP_ERR_PARSE, std::string("text string expected for ") + what);
        const uint8_t* q = take(h.arg);
        return std::string((const char*)q, (size_t)h.arg);
    }
    int64_t integer(const char* what) {
        const Head h = head();
        if (h.indef || h.arg > (uint64_t)INT64_MAX || h.major > 1) fail(ZKHIP_ERR_PARSE, std::string("integer expected for ") + what);
        return h.major == 0 ? (int64_t)h.arg : -1 - (int64_t)h.arg;
    }
    bool boolean(const char* what) {
        const uint8_t b = *take(1);
        if (b != 0xf4 && b != 0xf5) fail(ZKHIP_ERR_PARSE, std::string("boolean expected for ") + what);
        return b == 0xf5;
    }
};

// the statements as they are written: terms in stored order, nothing merged
struct RawTerm { int64_t id; uint32_t coeff; };
struct RawStatement {
    int kind = 0;                          // 0 constraint, 1 directive, 2 log (or anything else the constraint reader skips)
    uint32_t t0 = 0;                       // constraint: its three combinations are lc[t0 .. t0 + 3); directive: its 2 k input combinations
    uint32_t n_in = 0, o0 = 0, n_out = 0;  // directive: outputs are outs[o0 .. o0 + n_out)
    std::string solver;                    // directive: the variant's name
    uint64_t param = 0;                    // Bits(n), SnarkVerifyBls12377(n)
};

template <class P>
struct Compiler {
    typedef Fe<P> Fr;
    const zkhip_prog& prog;
    XPlanHost& out;
    std::vector<RawStatement> st;
    std::vector<RawTerm> terms;
    std::vector<std::pair<uint32_t, uint32_t>> lc;      // (first term, count)
    std::vector<int64_t> outs;
    std::map<std::array<uint32_t, 8>, uint32_t> coeff_of;
    // Computation::generate_constraints' allocation, replayed: the column of every id a constraint or a parameter names
    std::unordered_map<int64_t, uint32_t> tag;          // id -> instance index, or WIT | witness index
    std::vector<int64_t> inst, wit;
    static constexpr uint32_t WIT = 0x80000000u;
    struct Param { int64_t id; bool priv; uint32_t tag; };
    std::vector<Param> params;

    Compiler(const zkhip_prog& p, XPlanHost& o) : prog(p), out(o) {}

    uint32_t coefficient(const uint8_t* bytes) {
        std::array<uint32_t, 8> c;
        memcpy(c.data(), bytes, 32);
        Fr x;
        memcpy(x.v, bytes, 32);
        if (!canon_below_mod(x)) fail(ZKHIP_ERR_PARSE, "non-canonical field element in the program");
        auto it = coeff_of.find(c);
        if (it != coeff_of.end()) return it->second;
        const uint32_t k = (uint32_t)(out.pool.size() / 8);
        const Fr m = fe_to_mont(x);
        out.pool.insert(out.pool.end(), m.v, m.v + 8);
        coeff_of.emplace(c, k);
        return k;
    }
    static bool canon_below_mod(const Fr& x) {
        for (int i = P::N - 1; i >= 0; --i)
            if (x.v[i] != P::mod(i)) return x.v[i] < P::mod(i);
        return false;
    }
    void seed_pool() {
        uint8_t one[32] = {1};
        Fr m1 = fe_from_mont(fe_neg(Fr::one()));
        if (coefficient(one) != XCOEFF_ONE || coefficient((const uint8_t*)m1.v) != XCOEFF_MINUS_ONE) fail(ZKHIP_ERR_BAD_ARG, "internal: coefficient pool");
    }
    void see(int64_t id) {      // symbols.entry(k).or_insert_with(..)   zokrates_ark/src/lib.rs:50-70
        if (tag.count(id)) return;
        if (id < 0) { tag[id] = (uint32_t)inst.size(); inst.push_back(id); }
        else { tag[id] = WIT | (uint32_t)wit.size(); wit.push_back(id); }
        if (inst.size() + wit.size() >= (WIT >> 1)) fail(ZKHIP_ERR_BAD_ARG, "too many variables");
    }
    static int64_t variable_id(XCbor& c) {
        int64_t id = 0;
        bool have = false;
        uint64_t vf = c.enter(5, "a variable");
        while (c.more(vf)) {
            if (c.text("a Variable field") == "id") { id = c.integer("Variable.id"); have = true; }
            else c.skip();
        }
        if (!have) fail(ZKHIP_ERR_PARSE, "Variable without id");
        return id;
    }
    void lin_comb(XCbor& c, bool allocate) {
        const uint32_t first = (uint32_t)terms.size();
        uint64_t nf = c.enter(5, "a linear combination");
        bool have = false;
        while (c.more(nf)) {
            if (c.text("a LinComb field") != "value") { c.skip(); continue; }
            have = true;
            uint64_t nt = c.enter(4, "LinComb.value");
            while (c.more(nt)) {
                if (c.enter(4, "a (variable, coefficient) pair") != 2) fail(ZKHIP_ERR_PARSE, "LinComb term is not a pair");
                RawTerm t;
                t.id = variable_id(c);
                const XCbor::Head h = c.head();
                if (h.major != 2 || h.indef || h.arg != 32) fail(ZKHIP_ERR_PARSE, "field element is not a 32-byte string");
                t.coeff = coefficient(c.take(32));
                if (allocate) see(t.id);
                if (terms.size() >= 0xfffffff0u) fail(ZKHIP_ERR_BAD_ARG, "too many terms for a plan");
                terms.push_back(t);
            }
        }
        if (!have) fail(ZKHIP_ERR_PARSE, "LinComb without value");
        lc.push_back({first, (uint32_t)terms.size() - first});
    }
    void quad_comb(XCbor& c, bool allocate) {
        uint64_t qf = c.enter(5, "a quadratic combination");
        int seen = 0;
        while (c.more(qf)) {
            const std::string k = c.text("a QuadComb field");
            if (k == "left" && seen == 0) { lin_comb(c, allocate); seen = 1; }
            else if (k == "right" && seen == 1) { lin_comb(c, allocate); seen = 2; }
            else if (k == "left" || k == "right") fail(ZKHIP_ERR_PARSE, "QuadComb fields out of order");
            else c.skip();
        }
        if (seen != 2) fail(ZKHIP_ERR_PARSE, "QuadComb without left/right");
    }
    void constraint(XCbor& c, RawStatement& s) {
        s.kind = 0;
        s.t0 = (uint32_t)lc.size();
        uint64_t nf = c.enter(5, "a constraint statement");
        int seen = 0;
        while (c.more(nf)) {
            const std::string k = c.text("a ConstraintStatement field");
            if (k == "quad" && seen == 0) { quad_comb(c, true); seen = 1; }
            else if (k == "lin" && seen == 1) { lin_comb(c, true); seen = 2; }
            else if (k == "quad" || k == "lin") fail(ZKHIP_ERR_PARSE, "ConstraintStatement fields out of order");
            else c.skip();      // span, error
        }
        if (seen != 2) fail(ZKHIP_ERR_PARSE, "ConstraintStatement without quad/lin");
    }
    void solver(XCbor& c, RawStatement& s) {
        // a unit variant is a bare string, a newtype variant {name: payload}
        const uint8_t b = c.p < c.e ? *c.p : 0;
        if ((b >> 5) == 3) { s.solver = c.text("the solver"); return; }
        if (c.enter(5, "the solver") != 1) fail(ZKHIP_ERR_PARSE, "solver is not a single-entry map");
        s.solver = c.text("the solver variant");
        if (s.solver == "Bits" || s.solver == "SnarkVerifyBls12377") {
            const int64_t n = c.integer("the solver's width");
            if (n < 0) fail(ZKHIP_ERR_PARSE, "negative solver width");
            s.param = (uint64_t)n;
        } else {
            c.skip();
        }
    }
    void directive(XCbor& c, RawStatement& s) {
        s.kind = 1;
        s.t0 = (uint32_t)lc.size();
        s.o0 = (uint32_t)outs.size();
        uint64_t nf = c.enter(5, "a directive statement");
        bool have_solver = false;
        while (c.more(nf)) {
            const std::string k = c.text("a DirectiveStatement field");
            if (k == "inputs") {
                uint64_t ni = c.enter(4, "Directive.inputs");
                while (c.more(ni)) { quad_comb(c, false); ++s.n_in; }
            } else if (k == "outputs") {
                uint64_t no = c.enter(4, "Directive.outputs");
                while (c.more(no)) { outs.push_back(variable_id(c)); ++s.n_out; }
            } else if (k == "solver") {
                solver(c, s);
                have_solver = true;
            } else {
                c.skip();
            }
        }
        if (!have_solver) fail(ZKHIP_ERR_PARSE, "DirectiveStatement without solver");
    }
    void read_parameters(const uint8_t* b, uint64_t len) {
        XCbor c{b, b + len};
        tag[0] = 0;
        inst.push_back(0);      // symbols[~one] = ConstraintSystem::one()   lib.rs:89
        uint64_t np = c.enter(4, "the parameter list");
        while (c.more(np)) {
            uint64_t nf = c.enter(5, "a parameter");
            Param pr{0, false, 0};
            bool have_id = false, have_priv = false;
            while (c.more(nf)) {
                const std::string k = c.text("a Parameter field");
                if (k == "id") { pr.id = variable_id(c); have_id = true; }
                else if (k == "private") { pr.priv = c.boolean("Parameter.private"); have_priv = true; }
                else c.skip();
            }
            if (!have_id || !have_priv) fail(ZKHIP_ERR_PARSE, "Parameter without id/private");
            // `symbols.extend`: a repeated parameter takes a column of its own and re-binds the name   lib.rs:94-113
            if (pr.priv) { pr.tag = WIT | (uint32_t)wit.size(); wit.push_back(pr.id); }
            else { pr.tag = (uint32_t)inst.size(); inst.push_back(pr.id); }
            tag[pr.id] = pr.tag;
            params.push_back(pr);
        }
    }
    void read_statements(const uint8_t* b, uint64_t len) {
        XCbor c{b, b + len};
        while (c.p < c.e) {
            RawStatement s;
            if ((*c.p >> 5) == 3) { c.skip(); s.kind = 2; st.push_back(s); continue; }
            if (c.enter(5, "a statement") != 1) fail(ZKHIP_ERR_PARSE, "statement is not a single-entry map");
            const std::string variant = c.text("the statement variant");
            if (variant == "Constraint") constraint(c, s);
            else if (variant == "Directive") directive(c, s);
            else { c.skip(); s.kind = 2; }      // Log
            if (st.size() >= 0xfffffff0u) fail(ZKHIP_ERR_BAD_ARG, "too many statements for a plan");
            st.push_back(s);
        }
    }

    // ---- the compile pass
    uint64_t m = 0;
    std::vector<uint8_t> defined;                          // by slot
    std::unordered_map<int64_t, uint32_t> extra;           // ids without a column
    uint32_t column(uint32_t t) const { return (t & WIT) ? (uint32_t)(out.l + (t & ~WIT)) : t; }
    bool slot_of(int64_t id, uint32_t& slot) const {
        auto it = tag.find(id);
        if (it != tag.end()) { slot = column(it->second); return true; }
        auto ie = extra.find(id);
        if (ie != extra.end()) { slot = ie->second; return true; }
        return false;
    }
    uint32_t output_slot(int64_t id) {
        uint32_t slot;
        if (slot_of(id, slot)) return slot;
        slot = (uint32_t)(m + extra.size());
        if (slot >= 0xfffffff0u) fail(ZKHIP_ERR_BAD_ARG, "too many variables");
        extra.emplace(id, slot);
        defined.push_back(0);
        return slot;
    }
    void emit_lc(uint64_t k, uint64_t statement) {
        out.code.push_back(lc[k].second);
        for (uint32_t t = lc[k].first; t < lc[k].first + lc[k].second; ++t) {
            uint32_t slot;
            if (!slot_of(terms[t].id, slot) || !defined[slot])
                fail(ZKHIP_ERR_BAD_ARG, "statement " + std::to_string(statement) + " reads variable " + witness_var_name(terms[t].id) +
                                            " before anything defines it (the reference's interpreter would panic there)");
            out.code.push_back(slot);
            out.code.push_back(terms[t].coeff);
        }
    }
    void compile() {
        m = out.l + out.w;
        defined.assign(m, 0);
        defined[0] = 1;
        out.row_of.assign(st.size(), XPLAN_NO_ROW);
        // the arguments: a repeated parameter keeps its last value (Witness::insert), and each binding its own column
        for (size_t k = 0; k < params.size(); ++k) {
            const uint32_t slot = column(params[k].tag);
            out.code.push_back(XOP_ARG); out.code.push_back((uint32_t)k); out.code.push_back(slot);
            defined[slot] = 1;
        }
        uint64_t row = 0;
        for (size_t k = 0; k < st.size(); ++k) {
            const RawStatement& s = st[k];
            if (s.kind == 2) continue;
            ++out.n_statements;
            if (s.kind == 0) {
                out.row_of[k] = (uint32_t)row++;
                const std::pair<uint32_t, uint32_t> lin = lc[s.t0 + 2];
                uint32_t slot = 0;
                // is_assignee: ONE raw term, coefficient 1, a variable the witness does not hold yet   expression.rs:218-222
                const bool assignee = lin.second == 1 && terms[lin.first].coeff == XCOEFF_ONE && !(slot_of(terms[lin.first].id, slot) && defined[slot]);
                if (assignee) {
                    slot_of(terms[lin.first].id, slot);      // (a constraint's variable has a column)
                    out.code.push_back(XOP_DEFINE); out.code.push_back(slot);
                    emit_lc(s.t0, k); emit_lc(s.t0 + 1, k);
                    defined[slot] = 1;
                    ++out.n_defines;
                } else {
                    out.code.push_back(XOP_CHECK); out.code.push_back((uint32_t)k);
                    emit_lc(s.t0, k); emit_lc(s.t0 + 1, k); emit_lc(s.t0 + 2, k);
                    ++out.n_checks;
                }
                continue;
            }
            // a directive: Solver::get_signature   solvers.rs:52-69
            struct Sig { const char* name; uint32_t op; uint64_t n_in, n_out; };
            static const Sig sigs[] = {{"ConditionEq", XOP_CONDEQ, 1, 2}, {"Bits", XOP_BITS, 1, 0}, {"Div", XOP_DIV, 2, 1}, {"Xor", XOP_XOR, 2, 1},
                                       {"Or", XOP_OR, 2, 1}, {"ShaAndXorAndXorAnd", XOP_SHA3, 3, 1}, {"ShaCh", XOP_SHACH, 3, 1}, {"EuclideanDiv", XOP_EDIV, 2, 2}};
            const Sig* sig = nullptr;
            for (const Sig& g : sigs) if (s.solver == g.name) sig = &g;
            std::string shown = s.solver;
            for (char& ch : shown) if ((unsigned char)ch < 0x20 || (unsigned char)ch > 0x7e) ch = '?';
            if (!sig)
                fail(ZKHIP_ERR_BAD_ARG, "statement " + std::to_string(k) + ": a directive with the solver " + shown.substr(0, 64) +
                                            " keeps the host interpreter (on the device: ConditionEq, Bits, Div, Xor, Or, ShaAndXorAndXorAnd, ShaCh, EuclideanDiv)");
            const uint64_t want_out = sig->op == XOP_BITS ? s.param : sig->n_out;
            if (sig->op == XOP_BITS && s.param > XPLAN_MAX_BITS) fail(ZKHIP_ERR_BAD_ARG, "statement " + std::to_string(k) + ": Bits(" + std::to_string(s.param) + ") is wider than a plan takes");
            if (s.n_in != sig->n_in || s.n_out != want_out)
                fail(ZKHIP_ERR_BAD_ARG, "statement " + std::to_string(k) + ": the solver " + s.solver + " takes " + std::to_string(sig->n_in) + " inputs and gives " +
                                            std::to_string(want_out) + " outputs, the directive has " + std::to_string(s.n_in) + " and " + std::to_string(s.n_out));
            out.code.push_back(sig->op);
            if (sig->op == XOP_BITS) out.code.push_back((uint32_t)s.param);
            // the inputs are evaluated before any output is stored   lib.rs:87-106
            if (sig->op != XOP_BITS) {
                const size_t at = out.code.size();
                out.code.resize(at + s.n_out);
                for (uint32_t i = 0; i < 2 * s.n_in; ++i) emit_lc(s.t0 + i, k);
                for (uint32_t i = 0; i < s.n_out; ++i) out.code[at + i] = output_slot(outs[s.o0 + i]);
                for (uint32_t i = 0; i < s.n_out; ++i) defined[out.code[at + i]] = 1;
            } else {
                for (uint32_t i = 0; i < 2 * s.n_in; ++i) emit_lc(s.t0 + i, k);
                for (uint32_t i = 0; i < s.n_out; ++i) { const uint32_t sl = output_slot(outs[s.o0 + i]); out.code.push_back(sl); defined[sl] = 1; }
            }
            ++out.n_directives;
        }
        out.code.push_back(XOP_END);
        out.n_extra = extra.size();
        out.slots = m + extra.size();
        // the Witness at the end: every defined variable, by ascending signed id
        std::vector<std::pair<int64_t, uint32_t>> held;
        for (const auto& kv : tag) { const uint32_t sl = column(kv.second); if (defined[sl]) held.push_back({kv.first, sl}); }
        for (const auto& kv : extra) if (defined[kv.second]) held.push_back(kv);
        std::sort(held.begin(), held.end());
        for (const auto& h : held) { out.file_ids.push_back(h.first); out.file_slots.push_back(h.second); }
    }
};

template <class P>
void build(const zkhip_prog& prog, int curve, uint64_t l, uint64_t w, uint64_t n, const uint8_t* bytes, const uint64_t off[2], const uint64_t len[2], XPlanHost& out) {
    Compiler<P> c(prog, out);
    out.curve = curve; out.l = l; out.w = w; out.n = n;
    c.seed_pool();
    c.read_parameters(bytes + off[0], len[0]);
    c.read_statements(bytes + off[1], len[1]);
    // the program `prog` was parsed from: the same constraints, columns and arguments
    uint64_t constraints = 0;
    for (const auto& s : c.st) constraints += s.kind == 0;
    std::vector<int64_t> order = c.inst;
    order.insert(order.end(), c.wit.begin(), c.wit.end());
    std::vector<int64_t> pub;
    for (const auto& p : c.params) if (!p.priv) pub.push_back(p.id);
    if (constraints != prog.n || c.inst.size() != prog.l || c.wit.size() != prog.w || order != prog.order || pub != prog.public_args)
        fail(ZKHIP_ERR_BAD_ARG, "these `out` bytes are not the program the handle was parsed from (constraints " + std::to_string(constraints) + " / " +
                                    std::to_string(prog.n) + ", l " + std::to_string(c.inst.size()) + " / " + std::to_string(prog.l) + ", w " + std::to_string(c.wit.size()) + " / " +
                                    std::to_string(prog.w) + ", or another variable order or argument list)");
    out.n_args = c.params.size();
    c.compile();
    // where the public inputs sit: public arguments in argument order (each binding's own column), then ~out_0 .. ~out_{R-1}
    for (const auto& p : c.params) if (!p.priv) out.input_cols.push_back(c.column(p.tag));
    for (uint64_t k = 0; k < prog.return_count; ++k) {
        uint32_t slot;
        const int64_t id = -(int64_t)k - 1;
        if (!c.slot_of(id, slot) || !c.defined[slot]) fail(ZKHIP_ERR_BAD_ARG, "output " + witness_var_name(id) + " is never computed by the program");
        out.input_cols.push_back(slot);
    }
    xplan_schedule(out.code, out.slots, out.sched, out.level_start);
}

inline uint32_t rd32(const uint8_t* p) { uint32_t v; memcpy(&v, p, 4); return v; }
inline uint64_t rd64(const uint8_t* p) { uint64_t v; memcpy(&v, p, 8); return v; }

}  // namespace xplan_detail

// the plan of the program in `bytes` for a system of (curve, l, w, n constraints) that `prog` was parsed from; throws IngestError —
// ZKHIP_ERR_PARSE for bytes that are no program, ZKHIP_ERR_BAD_ARG naming why this program keeps the host interpreter
inline void xplan_build(const zkhip_prog& prog, int curve, uint64_t l, uint64_t w, uint64_t n, const uint8_t* bytes, size_t len, XPlanHost& out) {
    using namespace xplan_detail;
    if (prog.curve != curve) fail(ZKHIP_ERR_BAD_ARG, "the constraint system is over another curve than the program");
    if (prog.l != l || prog.w != w || prog.n != n)
        fail(ZKHIP_ERR_BAD_ARG, "the constraint system has n = " + std::to_string(n) + ", l = " + std::to_string(l) + ", w = " + std::to_string(w) + ", the program n = " +
                                    std::to_string(prog.n) + ", l = " + std::to_string(prog.l) + ", w = " + std::to_string(prog.w));
    // ProgHeader::read (serialize.rs:150-199), as zkhip_prog_parse reads it
    constexpr size_t HEADER = 20 + 4 * 20;
    static const uint8_t MAGIC_VERSION[8] = {0x5a, 0x4f, 0x4b, 0, 3, 0, 0, 0};
    static const uint8_t IDS[3][4] = {{0xb4, 0xf7, 0xb5, 0xbd}, {0x40, 0xd8, 0xc1, 0xf9}, {0xc2, 0x95, 0x5a, 0xb5}};
    if (len < HEADER || memcmp(bytes, MAGIC_VERSION, 8)) fail(ZKHIP_ERR_PARSE, "Invalid header");
    if (curve < 0 || curve > 2 || memcmp(bytes + 8, IDS[curve], 4)) fail(ZKHIP_ERR_BAD_ARG, "these `out` bytes are a program over another curve than the handle's");
    uint64_t off[2], ln[2];
    for (int s = 0; s < 2; ++s) {
        const uint8_t* q = bytes + 20 + 20 * s;
        off[s] = rd64(q + 4);
        ln[s] = rd64(q + 12);
        if (off[s] > len || ln[s] > len - off[s]) fail(ZKHIP_ERR_PARSE, "section outside the file");
    }
    if (rd32(bytes + 12) != prog.n || rd32(bytes + 16) != prog.return_count)
        fail(ZKHIP_ERR_BAD_ARG, "these `out` bytes are not the program the handle was parsed from (constraint or return count)");
    if (curve == ZKHIP_CURVE_BN128) build<Bn254Fr>(prog, curve, l, w, n, bytes, off, ln, out);
    else if (curve == ZKHIP_CURVE_BLS12_381) build<Bls381Fr>(prog, curve, l, w, n, bytes, off, ln, out);
    else build<Bls377Fr>(prog, curve, l, w, n, bytes, off, ln, out);
}

}  // namespace zk
