// exec_plan.cpp — the host side of witnesses computed on the device (csrc/xplan.h): the pass that compiles a program's statements into
// the instruction stream of k_exec_program, alone — no device, no library.  A well-formed program against the counts the test states,
// the stream walked word by word (every slot below the plan's slot count, every coefficient inside the pool, the stream ends where
// XOP_END stands), then every truncation of the file and single-byte mutations of its parameter and statement sections over heap
// blocks of exactly their sizes: each must end in a plan or an IngestError.  Built plain and under ASan + UBSan
// (tests/test_device_exec.py).
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -I zokrates_amd/csrc tests/host/exec_plan.cpp
//   exec_plan <out file> <curve> <n> <returns> <l> <w> <order, comma separated> <public argument ids> <7 expected dims>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>
#include <memory>
#include <sstream>

#include "xplan.h"

using namespace zk;

static int bad = 0;
static void expect(bool ok, const char* what, long long a = -1) {
    if (!ok) { printf("FAILED %s (%lld)\n", what, a); ++bad; }
}
static std::vector<int64_t> id_list(const char* s) {
    std::vector<int64_t> out;
    std::stringstream ss(s);
    std::string tok;
    while (std::getline(ss, tok, ',')) if (!tok.empty()) out.push_back(atoll(tok.c_str()));
    return out;
}
// the words of the stream: every one read stays inside it, every slot and coefficient inside the plan
static void walk(const XPlanHost& h) {
    size_t pc = 0;
    const size_t end = h.code.size();
    bool ok = true;
    auto word = [&]() -> uint32_t { if (pc >= end) { ok = false; return 0; } return h.code[pc++]; };
    auto slot = [&] { if (word() >= h.slots) ok = false; };
    auto lin = [&] { const uint32_t n = word(); for (uint32_t t = 0; t < n && ok; ++t) { slot(); if ((uint64_t)word() * 8 + 8 > h.pool.size()) ok = false; } };
    auto quad = [&] { lin(); lin(); };
    uint64_t defines = 0, checks = 0, directives = 0;
    while (ok) {
        const uint32_t op = word();
        if (op == XOP_END) break;
        switch (op) {
            case XOP_ARG: if (word() >= h.n_args) ok = false; slot(); break;
            case XOP_DEFINE: slot(); quad(); ++defines; break;
            case XOP_CHECK: { const uint32_t st = word(); if (st >= h.row_of.size() || h.row_of[st] == XPLAN_NO_ROW) ok = false; quad(); lin(); ++checks; break; }
            case XOP_CONDEQ: slot(); slot(); quad(); ++directives; break;
            case XOP_BITS: { const uint32_t n = word(); quad(); for (uint32_t i = 0; i < n && ok; ++i) slot(); ++directives; break; }
            case XOP_DIV: case XOP_XOR: case XOP_OR: slot(); quad(); quad(); ++directives; break;
            case XOP_SHA3: case XOP_SHACH: slot(); quad(); quad(); quad(); ++directives; break;
            case XOP_EDIV: slot(); slot(); quad(); quad(); ++directives; break;
            default: ok = false;
        }
    }
    expect(ok && pc == end, "the stream is well-formed and ends at XOP_END", (long long)pc);
    expect(defines == h.n_defines && checks == h.n_checks && directives == h.n_directives, "the stream holds the instructions the counts name");
    expect(h.file_ids.size() == h.file_slots.size() && std::is_sorted(h.file_ids.begin(), h.file_ids.end()), "the file's entries ascend by signed id");
    for (uint32_t s : h.file_slots) expect(s < h.slots, "a file entry's slot is inside the store", s);
    for (uint32_t s : h.input_cols) expect(s < h.slots, "an input's slot is inside the store", s);
}
// 1: a plan, 0: refused with an IngestError of a known code
static int attempt(const zkhip_prog& p, const uint8_t* bytes, size_t len) {
    std::unique_ptr<uint8_t[]> block(new uint8_t[len ? len : 1]);
    memcpy(block.get(), bytes, len);
    XPlanHost h;
    try {
        xplan_build(p, p.curve, p.l, p.w, p.n, block.get(), len, h);
    } catch (const IngestError& e) {
        expect((e.code == ZKHIP_ERR_PARSE || e.code == ZKHIP_ERR_BAD_ARG) && !e.msg.empty(), "a refusal is PARSE or BAD_ARG and says why", e.code);
        return 0;
    }
    walk(h);
    return 1;
}

int main(int argc, char** argv) {
    if (argc != 16) { printf("usage: exec_plan <out> <curve> <n> <returns> <l> <w> <order> <public args> <7 dims>\n"); return 2; }
    std::ifstream f(argv[1], std::ios::binary);
    std::vector<uint8_t> file((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    zkhip_prog p;
    p.curve = atoi(argv[2]); p.n = strtoull(argv[3], nullptr, 10); p.return_count = strtoull(argv[4], nullptr, 10);
    p.l = strtoull(argv[5], nullptr, 10); p.w = strtoull(argv[6], nullptr, 10);
    p.order = id_list(argv[7]);
    p.public_args = id_list(argv[8]);
    // ---- the program as it is
    XPlanHost h;
    try {
        xplan_build(p, p.curve, p.l, p.w, p.n, file.data(), file.size(), h);
    } catch (const IngestError& e) {
        printf("FAILED the well-formed program is refused: %s\n", e.msg.c_str());
        return 1;
    }
    uint64_t d[8];
    h.dims(d);
    for (int k = 0; k < 7; ++k) expect(d[k] == strtoull(argv[9 + k], nullptr, 10), "zkhip_xplan_dims", (long long)k * 1000000 + (long long)d[k]);
    expect(d[7] == 32 * (p.l + p.w + d[6]), "bytes of value store per instance");
    expect(h.slots == p.l + p.w + d[6], "slots");
    walk(h);
    // ---- another system or program than the handle's
    {
        zkhip_prog q = p;
        q.n += 1;
        expect(attempt(q, file.data(), file.size()) == 0, "another constraint count is refused");
        q = p; q.order.back() += 1;
        expect(attempt(q, file.data(), file.size()) == 0, "another variable order is refused");
        q = p; q.public_args.push_back(99);
        expect(attempt(q, file.data(), file.size()) == 0, "another argument list is refused");
        q = p; q.curve = (p.curve + 1) % 3;
        expect(attempt(q, file.data(), file.size()) == 0, "another curve is refused");
    }
    // ---- every truncation: none that cuts the parameters or the statements gives a plan (the sections behind them are not read)
    uint64_t off[2], ln[2];
    for (int s = 0; s < 2; ++s) { memcpy(&off[s], file.data() + 24 + 20 * s, 8); memcpy(&ln[s], file.data() + 32 + 20 * s, 8); }
    long plans = 0;
    for (size_t len = 0; len < file.size(); ++len) {
        const int got = attempt(p, file.data(), len);
        if (len < off[1] + ln[1]) plans += got;
    }
    expect(plans == 0, "no file cut inside its statements gives a plan", plans);
    // ---- single-byte mutations of the parameter and statement sections (and of the header's section table)
    long tried = 0;
    std::vector<uint8_t> m = file;
    auto mutate = [&](size_t at) {
        static const uint8_t flips[] = {0x01, 0x20, 0x80, 0xff, 0x1f};
        for (uint8_t x : flips) {
            m[at] = file[at] ^ x;
            plans += attempt(p, m.data(), m.size());
            ++tried;
        }
        m[at] = file[at];
    };
    for (size_t at = 8; at < 100; ++at) mutate(at);
    for (int s = 0; s < 2; ++s)
        for (size_t at = off[s]; at < off[s] + ln[s]; ++at) mutate(at);
    expect(tried > 1000, "the sweep covered the sections", tried);
    printf("%ld mutations, %ld of them still a plan\n%d failures\n", tried, plans, bad);
    return bad ? 1 : 0;
}
