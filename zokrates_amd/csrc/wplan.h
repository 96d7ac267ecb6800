// wplan.h — the host side of witness files read on the device (include/zkhip.h "witness files on the device"): the column order of a
// program as two lookup tables, where its public inputs sit in z, and the checks of a `witness` file that need no pass over its
// entries.  Pure host code over ingest.h's zkhip_prog (tests/host/witness_plan.cpp compiles it alone); the kernels that use the
// tables are in wingest.cuh, the resident plan and the entry points in core.cuh / zkhip_api.hip.
#pragma once
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/zkhip.h"
#include "ingest.h"

namespace zk {

static constexpr uint32_t WPLAN_NO_COLUMN = 0xffffffffu;      // a table entry of an id the system has no column for

// what a plan knows on the host
struct WPlanTables {
    int curve = 0;
    uint64_t l = 0, w = 0, returns = 0;
    std::vector<uint32_t> pos, neg;        // column of id k >= 0 at pos[k]; of id -(k + 1) at neg[k]; each as long as the largest id named + 1
    std::vector<int64_t> order;            // the program's: id of column j (names a missing column)
    std::vector<uint32_t> input_cols;      // public arguments in argument order, then ~out_0 .. ~out_{R-1}: all below l
};

// the reader's spelling of a variable (prog_assignment)
inline std::string witness_var_name(int64_t id) {
    return id == 0 ? std::string("~one") : id > 0 ? "_" + std::to_string(id - 1) : "~out_" + std::to_string(-(id + 1));
}
// the reader's range rule: an id whose index (id, or -(id + 1)) is at or above this is refused
inline uint64_t witness_id_bound(uint64_t count) {
    return std::min<uint64_t>((uint64_t)1 << 31, std::max<uint64_t>((uint64_t)1 << 20, 64 * count));
}
// Witness::read's framing, with the reader's messages: usize count, then count x 40 bytes.  Returns the count; throws IngestError
inline uint64_t witness_header_validate(const uint8_t* wit, size_t len) {
    if (len < 8) throw IngestError{ZKHIP_ERR_PARSE, "witness file truncated"};
    uint64_t count;
    memcpy(&count, wit, 8);
    if (count > (len - 8) / 40 || len != 8 + 40 * count) throw IngestError{ZKHIP_ERR_PARSE, "witness file size does not match its entry count"};
    // (an entry's index + 1 is what the kernels keep per column, in 32 bits)
    if (count >= 0xffffffffull) throw IngestError{ZKHIP_ERR_PARSE, "witness file has more entries than a plan can index"};
    return count;
}
// the tables of `prog` for a system of (curve, l, w); throws IngestError{ZKHIP_ERR_BAD_ARG} naming why this program keeps the host reader
inline void wplan_build(const zkhip_prog& prog, int curve, uint64_t l, uint64_t w, WPlanTables& out) {
    auto refuse = [](const std::string& why) { throw IngestError{ZKHIP_ERR_BAD_ARG, why}; };
    if (prog.curve != curve) refuse("the constraint system is over another curve than the program");
    if (prog.l != l || prog.w != w)
        refuse("the constraint system has l = " + std::to_string(l) + ", w = " + std::to_string(w) + ", the program l = " + std::to_string(prog.l) + ", w = " + std::to_string(prog.w));
    const uint64_t m = l + w;
    if (prog.order.size() != m || m == 0 || m >= WPLAN_NO_COLUMN) refuse("the program's variable order does not cover its columns");
    // ids the reader could never be given (its range rule over a file of about m entries) would only size the tables
    const uint64_t id_cap = witness_id_bound(m);
    uint64_t npos = 1, nneg = 0;
    for (uint64_t j = 0; j < m; ++j) {
        const int64_t id = prog.order[j];
        const uint64_t k = id >= 0 ? (uint64_t)id : (uint64_t)(-(id + 1));
        if (k >= id_cap) refuse("variable " + witness_var_name(id) + " has an id no witness file of this program's size may name");
        (id >= 0 ? npos : nneg) = std::max(id >= 0 ? npos : nneg, k + 1);
    }
    nneg = std::max<uint64_t>(nneg, prog.return_count);
    out.curve = curve; out.l = l; out.w = w; out.returns = prog.return_count;
    out.pos.assign(npos, WPLAN_NO_COLUMN);
    out.neg.assign(nneg, WPLAN_NO_COLUMN);
    out.order = prog.order;
    for (uint64_t j = 0; j < m; ++j) {
        const int64_t id = prog.order[j];
        uint32_t& slot = id >= 0 ? out.pos[(uint64_t)id] : out.neg[(uint64_t)(-(id + 1))];
        if (slot != WPLAN_NO_COLUMN)
            refuse("variable " + witness_var_name(id) + " sits at columns " + std::to_string(slot) + " and " + std::to_string(j) +
                   ": its assignment would be consumed twice (repeated parameter)");
        slot = (uint32_t)j;
    }
    auto column = [&](int64_t id, const char* what) -> uint32_t {
        const std::vector<uint32_t>& t = id >= 0 ? out.pos : out.neg;
        const uint64_t k = id >= 0 ? (uint64_t)id : (uint64_t)(-(id + 1));
        const uint32_t c = k < t.size() ? t[k] : WPLAN_NO_COLUMN;
        if (c == WPLAN_NO_COLUMN) refuse(std::string(what) + " " + witness_var_name(id) + " has no column");
        if (c >= l) refuse(std::string(what) + " " + witness_var_name(id) + " is not an instance column");
        return c;
    };
    out.input_cols.clear();
    for (int64_t id : prog.public_args) out.input_cols.push_back(column(id, "public argument"));
    for (uint64_t k = 0; k < prog.return_count; ++k) out.input_cols.push_back(column(-(int64_t)k - 1, "output"));
}

}  // namespace zk
