// staged_out_check.cpp -- stand-alone check of StagedOuts + Bump (csrc/capi_staged_out.hpp): every slice handed out is 256-byte
// aligned, lies inside [base, base + bytes()) and overlaps no other; an output that is not staged keeps the caller's pointer and
// adds no bytes.  The block is allocated with exactly bytes() bytes and every slice is written in full, so an address sanitizer
// sees a slice that leaves it.  Built and run by tests/test_staged_out_cpu.py with -fsanitize=address,undefined.
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>
#include <vector>

#include "../polars_ds_extension_amd/csrc/capi_staged_out.hpp"

static int failures = 0;
#define CHECK(cond, what)                                                      \
    do {                                                                       \
        if (!(cond)) {                                                         \
            std::printf("FAIL %s: %s (line %d)\n", what, #cond, __LINE__);     \
            ++failures;                                                        \
        }                                                                      \
    } while (0)

// place the sets one after the other into a block of exactly their bytes; n_staged / n_back: what the declaration must give
static void check(const char* what, std::vector<StagedOuts*> sets, int n_staged, int n_back, size_t want_bytes) {
    size_t bytes = 0;
    for (StagedOuts* s : sets) bytes += s->bytes();
    CHECK(bytes == want_bytes, what);
    CHECK(bytes % 256 == 0, what);
    char* base = static_cast<char*>(std::aligned_alloc(256, std::max<size_t>(bytes, 256)));
    char* block = bytes ? base : nullptr;  // (nothing staged: nothing may be taken)
    Bump w{block};
    std::vector<std::pair<char*, char*>> slices;
    int staged = 0, back = 0;
    for (StagedOuts* s : sets) {
        std::vector<void*> users;
        for (int i = 0; i < s->n; ++i) users.push_back(s->dev(i));  // (add() has set the device pointer to the caller's)
        for (int i = 0; i < s->n; ++i) CHECK(users[i] == s->outs[i].user, what);
        s->place(w);
        for (int i = 0; i < s->n; ++i) {
            const StagedOuts::Out& o = s->outs[i];
            char* d = static_cast<char*>(s->dev(i));
            back += o.back;
            if (!o.staged) {
                CHECK(d == o.user, what);
                CHECK(o.room == 0 || (s->stage && !o.user), what);  // (only kOutRoom keeps room for an absent output)
                CHECK(!o.back, what);
                continue;
            }
            ++staged;
            const size_t len = s->cap * o.unit_bytes;
            CHECK(o.room == Bump::up(len), what);
            CHECK(reinterpret_cast<uintptr_t>(d) % 256 == 0, what);
            CHECK(d >= block && d + len <= block + bytes, what);
            CHECK(!o.back || (s->host && o.user), what);
            if (!len) continue;  // (an empty slice touches nothing)
            std::memset(d, 0xA5, len);
            slices.push_back({d, d + len});
        }
    }
    CHECK(w.p <= block + bytes, what);
    CHECK(staged == n_staged && back == n_back, what);
    std::sort(slices.begin(), slices.end());
    for (size_t i = 1; i < slices.size(); ++i) CHECK(slices[i - 1].second <= slices[i].first, what);
    std::free(base);
}

template <typename T>
static void report(bool host, size_t cap, int pp) {
    static T buf[9];  // (stand-ins for the caller's buffers: only their addresses are used)
    T* d[8];
    uint8_t flag, *d_flag;
    StagedOuts so(host, cap);
    for (int i = 0; i < 6; ++i) so.add(&d[i], &buf[i], pp);
    so.add(&d[6], &buf[6], 1);
    so.add(&d[7], &buf[7], 1);
    so.add(&d_flag, &flag, 1);
    const size_t want = host ? 6 * Bump::up(cap * pp * sizeof(T)) + 2 * Bump::up(cap * sizeof(T)) + Bump::up(cap) : 0;
    check("report", {&so}, host ? 9 : 0, host ? 9 : 0, want);
}

template <typename T>
static void glm(bool host, bool per_row, StagedOuts::Kind kind, size_t cap, size_t n_rows, int pp) {
    T co, pr, *d_co, *d_pr;
    int32_t it, *d_it;
    uint8_t nu, rn, *d_nu, *d_rn;
    StagedOuts g(host, cap), r(host, n_rows);
    g.add(&d_co, &co, pp);
    g.add(&d_it, &it, 1);
    g.add(&d_nu, &nu, 1);
    r.add(&d_pr, per_row ? &pr : (T*)nullptr, 1, kind);
    r.add(&d_rn, per_row ? &rn : (uint8_t*)nullptr, 1, kind);
    size_t want = 0;
    if (host) want = Bump::up(cap * pp * sizeof(T)) + Bump::up(cap * 4) + Bump::up(cap);
    if (host && (per_row || kind == StagedOuts::kOutRoom)) want += Bump::up(n_rows * sizeof(T)) + Bump::up(n_rows);
    const int n = host ? 3 + (per_row ? 2 : 0) : 0;
    check("glm", {&g, &r}, n, n, want);
    if (!per_row) CHECK(d_pr == nullptr && d_rn == nullptr, "glm: an absent output has no device pointer");
}

int main() {
    for (size_t cap : {37, 64}) {
        report<double>(true, cap, 4);
        report<float>(true, cap, 3);
        report<double>(false, cap, 4);
    }
    for (bool host : {true, false})
        for (bool per_row : {true, false})
            for (StagedOuts::Kind kind : {StagedOuts::kOut, StagedOuts::kOutRoom}) {
                glm<double>(host, per_row, kind, 37, 1531, 4);
                glm<float>(host, per_row, kind, 64, 1531, 3);
            }
    {  // "stage when the caller gave none" on a device frame: coefficients absent, flags given; and both absent; and a host frame
        double co, *d_co;
        uint8_t nu, *d_nu;
        StagedOuts a(false, 37);
        a.add(&d_co, (double*)nullptr, 4, StagedOuts::kScratch);
        a.add(&d_nu, &nu, 1, StagedOuts::kScratch);
        check("scratch, device, no coeffs", {&a}, 1, 0, Bump::up(37 * 4 * 8));
        CHECK(d_co != nullptr && d_nu == &nu, "scratch, device, no coeffs");
        StagedOuts b(false, 37);
        b.add(&d_co, (double*)nullptr, 4, StagedOuts::kScratch);
        b.add(&d_nu, (uint8_t*)nullptr, 1, StagedOuts::kScratch);
        check("scratch, device, nothing given", {&b}, 2, 0, Bump::up(37 * 4 * 8) + 256);
        StagedOuts c(true, 37);
        c.add(&d_co, &co, 4, StagedOuts::kScratch);
        c.add(&d_nu, (uint8_t*)nullptr, 1, StagedOuts::kScratch);
        check("scratch, host", {&c}, 2, 1, Bump::up(37 * 4 * 8) + 256);
        StagedOuts d(false, 37);
        d.add(&d_co, &co, 4, StagedOuts::kScratch);
        d.add(&d_nu, &nu, 1, StagedOuts::kScratch);
        check("scratch, device, all given", {&d}, 0, 0, 0);
        CHECK(d_co == &co && d_nu == &nu, "scratch, device, all given");
    }
    for (size_t cap : {0, 1, 255, 256, 257}) {  // slices of 0, 1 and 255 / 256 / 257 bytes, between wider ones
        double x, *d_x;
        uint8_t a, b, *d_a, *d_b;
        StagedOuts so(true, cap);
        so.add(&d_a, &a, 1);
        so.add(&d_x, &x, 3);
        so.add(&d_b, &b, 1);
        check("byte counts", {&so}, 3, 3, 2 * Bump::up(cap) + Bump::up(cap * 24));
    }
    for (bool host : {true, false}) {  // results rearranged on the device: the fit's set is staged on a device frame too
        double co, *d_co, *o_co;
        uint8_t va, *d_va, *o_va;
        StagedOuts fit(host, 1531, true), scattered(host, 1531);
        fit.add(&d_co, &co, 4);
        fit.add(&d_va, &va, 1);
        scattered.add(&o_co, &co, 4);
        scattered.add(&o_va, &va, 1);
        const size_t one = Bump::up(1531 * 4 * 8) + Bump::up(1531);
        check("scatter", {&fit, &scattered}, host ? 4 : 2, host ? 4 : 0, host ? 2 * one : one);
        if (!host) CHECK(o_co == &co && o_va == &va && d_co != &co, "scatter");
    }
    if (failures) return 1;
    std::printf("staged_out_check ok\n");
    return 0;
}
