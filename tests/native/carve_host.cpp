// Host check of the query scratch layouts (kubernetes-simulator_amd/csrc/ks_carve.h), for CPU tests
// only.  For the edge counts of ks_place_at (k pods), ks_drain_at (n_ev evicted pods, nb candidate
// blocks) and the per-node lists (n nodes), ks_host_carve_check() runs every layout twice as the
// entry points do — a sizing pass, then a pass over a buffer of exactly that size — and checks that
//   * every range lies inside the reserved size and no two overlap (each range is also written, so a
//     build with -fsanitize=address sees a range that leaves the buffer);
//   * PodRec ranges start on 16 bytes, every other range on its element's alignment;
//   * every offset is the one the formulas below give: the word offsets ks_place_at and ks_drain_at
//     used before the layouts were shared, restated independently.
// It returns the number of violated checks.  With -DKS_CARVE_MAIN the file is a stand-alone program
// (for a sanitizer build: -fsanitize=address,undefined on the host side).  Not part of the product.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../kubernetes-simulator_amd/csrc/ks_carve.h"

namespace {

using ks_host::Carve;

constexpr int64_t W = 6, PW = 3, EW = 5, S = 64, L = ks::kPlaceL;  // words of PodRec, Placement, Eviction
static_assert(sizeof(ks::PodRec) == 8 * W && sizeof(ks::Placement) == 8 * PW && sizeof(ks::Eviction) == 8 * EW &&
              ks::kPlaceMaxShapes == S && ks::kPlaceMaxPods == 1024, "record sizes");

struct Range {
    const char* name;
    const void* p;
    int64_t bytes, align, want_off;  // want_off: the expected offset in words of the scratch
};

struct Checker {
    int64_t bad = 0;
    void fail(const char* what, const char* name, int64_t a, int64_t b) {
        if (bad++ < 20) std::fprintf(stderr, "carve: %s: %s (%lld, %lld)\n", name, what, (long long)a, (long long)b);
    }
    // ranges of one scratch of `words` words of `word` bytes at base
    void check(char* base, int64_t word, int64_t words, const std::vector<Range>& rs) {
        for (const Range& r : rs) {
            const int64_t off = (const char*)r.p - base;
            if (off < 0 || off + r.bytes > words * word) fail("outside the reserved size", r.name, off, r.bytes);
            else std::memset(base + off, 0x5A, r.bytes);
            if (off % r.align) fail("misaligned", r.name, off, r.align);
            if (off != r.want_off * word) fail("offset differs from the formula", r.name, off, r.want_off * word);
            for (const Range& q : rs)
                if (&q != &r && r.bytes && q.bytes && (const char*)q.p < (const char*)r.p + r.bytes &&
                    (const char*)r.p < (const char*)q.p + q.bytes)
                    fail("overlaps", r.name, off, (const char*)q.p - base);
        }
    }
};

int64_t even(int64_t x) { return (x + 1) & ~(int64_t)1; }

void check_place(Checker& c, int64_t n, int64_t k) {
    const int64_t np = (n + 63) / 64 * 64, nblk = (n + 255) / 256;
    Carve qs(8), qi(4);
    ks_host::carve_place_at(qs, qi, n, np, nblk, k);
    // 16-byte aligned, as hipMalloc's
    std::vector<long double> m_qs((qs.at * 8 + 15) / 16 + 1), m_qi((qi.at * 4 + 15) / 16 + 1);
    const int64_t w_qs = qs.at, w_qi = qi.at;
    qs = Carve(8, m_qs.data());
    qi = Carve(4, m_qi.data());
    const ks_host::PlaceScratch s = ks_host::carve_place_at(qs, qi, n, np, nblk, k);
    if (qs.at != w_qs || qi.at != w_qi) c.fail("the two passes differ", "place", qs.at, w_qs);
    // the formulas of ks_place_at
    const int64_t up_words = W * S + (k + 1) / 2, rb_words = 2 + PW * k;
    const int64_t o_up = 4 * np, o_lists = o_up + up_words, o_top = o_lists + S * nblk * L, o_cc = o_top + S * L;
    const int64_t o_down = o_cc + S, o_after = o_down + rb_words;
    if (w_qs != o_after + 4 * n) c.fail("reserved size differs from the formula", "place d_qs", w_qs, o_after + 4 * n);
    if (w_qi != S * nblk) c.fail("reserved size differs from the formula", "place d_qi", w_qi, S * nblk);
    c.check((char*)m_qs.data(), 8, w_qs,
            {{"state", s.b.state, 32 * np, 8, 0},
             {"shapes", s.b.shapes, 8 * W * S, 16, o_up},
             {"shape_of", s.b.shape_of, 4 * k, 4, o_up + W * S},
             {"lists", s.b.lists, 8 * S * nblk * L, 8, o_lists},
             {"top", s.b.top, 8 * S * L, 8, o_top},
             {"ccount", s.b.ccount, 8 * S, 8, o_cc},
             {"rb", s.b.rb, 16, 4, o_down},
             {"out", s.b.out, 8 * PW * k, 8, o_down + 2},
             {"after", s.after, 32 * n, 8, o_after}});
    c.check((char*)m_qi.data(), 4, w_qi, {{"cnt", s.b.cnt, 4 * S * nblk, 4, 0}});
    if (s.b.n_pad != np) c.fail("n_pad", "place", s.b.n_pad, np);
}

void check_drain(Checker& c, int64_t n, int64_t n_ev, int64_t nb) {
    const int64_t np = (n + 63) / 64 * 64, nblk = (n + 255) / 256, CW = (n + 31) / 32;
    Carve qi(4);
    ks_host::carve_drain_gather(qi, CW, nb, nblk);
    std::vector<long double> m_qi((qi.at * 4 + 15) / 16 + 1);
    const int64_t w_qi = qi.at;
    qi = Carve(4, m_qi.data());
    ks_host::DrainGather g = ks_host::carve_drain_gather(qi, CW, nb, nblk);
    // the formulas of ks_drain_at: the int32 scratch ...
    const int64_t o_bcnt = CW, o_boff = o_bcnt + nb, o_total = even(o_boff + nb), o_cnt = o_total + 2;
    if (qi.at != w_qi || w_qi != o_cnt + S * nblk) c.fail("reserved size differs from the formula", "drain d_qi", w_qi, o_cnt + S * nblk);
    c.check((char*)m_qi.data(), 4, w_qi,
            {{"cordon", g.d.cordon, 4 * CW, 4, 0},
             {"bcnt", g.d.bcnt, 4 * nb, 4, o_bcnt},
             {"boff", g.d.boff, 4 * nb, 4, o_boff},
             {"total", g.d.total, 8, 8, o_total},
             {"cnt", g.cnt, 4 * S * nblk, 4, o_cnt}});
    // ... and the 64-bit scratch, sized from the total
    Carve qs(8);
    ks_host::carve_drain(qs, n, np, nblk, n_ev, &g.d);
    std::vector<long double> m_qs((qs.at * 8 + 15) / 16 + 1);
    const int64_t w_qs = qs.at;
    qs = Carve(8, m_qs.data());
    const ks_host::DrainScratch s = ks_host::carve_drain(qs, n, np, nblk, n_ev, &g.d);
    const int64_t up_words = W * S + (1024 + 1) / 2;
    int64_t o = 0;
    const int64_t o_state = o;   o += 4 * np;
    const int64_t o_up = o;      o += up_words;
    const int64_t o_lists = o;   o += S * nblk * L;
    const int64_t o_top = o;     o += S * L;
    const int64_t o_cc = o;      o += S;
    const int64_t o_rb = o;      o += 2;
    const int64_t o_placed = o;  o += PW * n_ev;
    const int64_t o_pod = o;     o += n_ev;
    const int64_t o_from = o;    o = even(o + (n_ev + 1) / 2);
    const int64_t o_rec = o;     o += W * n_ev;
    const int64_t o_evict = o;   o += EW * n_ev;
    const int64_t o_after = o;   o += 4 * n;
    if (qs.at != w_qs || w_qs != o) c.fail("reserved size differs from the formula", "drain d_qs", w_qs, o);
    c.check((char*)m_qs.data(), 8, w_qs,
            {{"state", s.b.state, 32 * np, 8, o_state},
             {"shapes", s.b.shapes, 8 * W * S, 16, o_up},
             {"shape_of", s.b.shape_of, 4 * 1024, 4, o_up + W * S},
             {"lists", s.b.lists, 8 * S * nblk * L, 8, o_lists},
             {"top", s.b.top, 8 * S * L, 8, o_top},
             {"ccount", s.b.ccount, 8 * S, 8, o_cc},
             {"rb", s.b.rb, 16, 16, o_rb},
             {"placed", s.b.out, 8 * PW * n_ev, 16, o_placed},
             {"ev_pod", g.d.ev_pod, 8 * n_ev, 8, o_pod},
             {"ev_from", g.d.ev_from, 4 * n_ev, 4, o_from},
             {"ev_rec", g.d.ev_rec, 8 * W * n_ev, 16, o_rec},
             {"evict", s.evict, 8 * EW * n_ev, 16, o_evict},
             {"after", s.after, 32 * n, 8, o_after}});
    if (g.d.cap != n_ev || s.b.n_pad != np) c.fail("cap / n_pad", "drain", g.d.cap, s.b.n_pad);
}

void check_node_lists(Checker& c, int64_t n, int64_t cap) {
    Carve qi(4);
    ks_host::carve_node_lists(qi, n, cap);
    std::vector<long double> m((qi.at * 4 + 15) / 16 + 1);
    const int64_t w = qi.at;
    qi = Carve(4, m.data());
    const ks_host::NodeLists l = ks_host::carve_node_lists(qi, n, cap);
    if (qi.at != w || w != 3 * n + 1 + cap) c.fail("reserved size differs from the formula", "node lists", w, 3 * n + 1 + cap);
    c.check((char*)m.data(), 4, w,
            {{"off", l.off, 4 * (n + 1), 4, 0},
             {"cur", l.cur, 4 * n, 4, n + 1},
             {"cnt", l.cnt, 4 * n, 4, 2 * n + 1},
             {"list", l.list, 4 * cap, 4, 3 * n + 1}});
}

}  // namespace

extern "C" int64_t ks_host_carve_check() {
    Checker c;
    for (int64_t n : {1, 255, 256, 257, 600}) {
        for (int64_t k : {1, 2, 33, 1024}) check_place(c, n, k);
        for (int64_t n_ev : {0, 1, 3, 65536})
            for (int64_t nb : {0, 1, 2, 7}) check_drain(c, n, n_ev, nb);
        for (int64_t cap : {0, 256, 7 * 256}) check_node_lists(c, n, cap);
    }
    return c.bad;
}

#ifdef KS_CARVE_MAIN
int main() {
    const int64_t bad = ks_host_carve_check();
    std::printf("carve check: %lld violated\n", (long long)bad);
    return bad != 0;
}
#endif
