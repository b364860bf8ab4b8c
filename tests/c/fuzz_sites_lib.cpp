// fuzz_sites_lib.cpp -- the host half of the library site profiles (rnascan_amd/csrc/pfmscan_sites_lib_host.hip, host only)
// under the sanitizers: random and adversarial motif-major hit lists, record tables and value lists in exact-size heap
// buffers.  pfmscan_site_groups_lib is checked against one pfmscan_site_groups call per motif (the definition), the order
// against std::stable_sort, the long accumulators against their invariants: one value rounds back to itself, v + v is 2 v,
// two halves merged are the whole, limb by limb, and stay normalised.  (The comparison with math.fsum is
// tests/test_sites_lib_cpu.py's.)  Built and run by that file with g++ -fsanitize=address,undefined.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <random>
#include <vector>

#include "pfmscan.h"

static int failures = 0;
#define CHECK(cond)                                                    \
    do {                                                               \
        if (!(cond)) {                                                 \
            std::printf("line %d: %s\n", __LINE__, #cond);             \
            if (++failures > 20) std::exit(1);                         \
        }                                                              \
    } while (0)

// exact-size heap copy: one element past the end is the sanitizer's
template <typename T> static T *heap(const std::vector<T> &v)
{
    T *p = static_cast<T *>(std::malloc(v.size() ? v.size() * sizeof(T) : 1));
    if (!v.empty()) std::memcpy(p, v.data(), v.size() * sizeof(T));
    return p;
}
template <typename T> static T *room(size_t n) { return static_cast<T *>(std::malloc(n ? n * sizeof(T) : 1)); }

// the definition: every motif's own list through pfmscan_site_groups
static bool by_definition(const std::vector<int64_t> &pos, const std::vector<int32_t> &mot, int n_motifs, const std::vector<int64_t> &off,
                          const std::vector<int64_t> &len, int m, std::vector<int64_t> &wf, std::vector<int64_t> &wr,
                          std::vector<int64_t> &wm)
{
    wf.clear(), wr.clear(), wm.clear();
    for (size_t h = 0; h < mot.size(); ++h)
        if (mot[h] < 0 || mot[h] >= n_motifs || (h > 0 && mot[h] < mot[h - 1])) return false;
    int64_t none = 0, n = 0;
    if (pfmscan_site_groups(nullptr, 0, off.data(), len.data(), (int64_t)off.size(), m, 0, &none, nullptr, &n) != PFMSCAN_OK) return false;
    for (size_t a = 0; a < pos.size();) {
        size_t b = a;
        while (b < pos.size() && mot[b] == mot[a]) ++b;
        std::vector<int64_t> f(b - a + 1), r(b - a);
        if (pfmscan_site_groups(pos.data() + a, (int64_t)(b - a), off.data(), len.data(), (int64_t)off.size(), m, (int64_t)(b - a),
                                f.data(), r.data(), &n) != PFMSCAN_OK)
            return false;
        for (int64_t g = 0; g < n; ++g) {
            wf.push_back(f[(size_t)g] + (int64_t)a);
            wr.push_back(r[(size_t)g]);
            wm.push_back(mot[a]);
        }
        a = b;
    }
    wf.push_back((int64_t)pos.size());
    return true;
}

static void one(const std::vector<int64_t> &pos, const std::vector<int32_t> &mot, int n_motifs, const std::vector<int64_t> &off,
                const std::vector<int64_t> &len, int m)
{
    std::vector<int64_t> wf, wr, wm;
    const bool ok = by_definition(pos, mot, n_motifs, off, len, m, wf, wr, wm);
    int64_t *hp = heap(pos), *ho = heap(off), *hl = heap(len);
    int32_t *hm = heap(mot);
    const int64_t n_hits = (int64_t)pos.size(), n_rec = (int64_t)off.size();
    int64_t n = -7;
    int64_t *first0 = room<int64_t>(1);
    int rc = pfmscan_site_groups_lib(hp, hm, n_hits, n_motifs, ho, hl, n_rec, m, 0, first0, nullptr, nullptr, &n);
    if (!ok) {
        CHECK(rc == PFMSCAN_E_BADARG);
    } else {
        CHECK(n == (int64_t)wr.size());
        CHECK(rc == (wr.empty() ? PFMSCAN_OK : PFMSCAN_E_CAPACITY));
        if (!wr.empty()) {                                  // one short: still refused, nothing written
            int64_t *f = room<int64_t>(wr.size()), *g = room<int64_t>(wr.size() - 1), *k = room<int64_t>(wr.size() - 1);
            CHECK(pfmscan_site_groups_lib(hp, hm, n_hits, n_motifs, ho, hl, n_rec, m, (int64_t)wr.size() - 1, f, g, k, &n) == PFMSCAN_E_CAPACITY);
            CHECK(n == (int64_t)wr.size());
            std::free(f), std::free(g), std::free(k);
        }
        int64_t *f = room<int64_t>(wr.size() + 1), *g = room<int64_t>(wr.size()), *k = room<int64_t>(wr.size());
        rc = pfmscan_site_groups_lib(hp, hm, n_hits, n_motifs, ho, hl, n_rec, m, (int64_t)wr.size(), f, g, k, &n);
        CHECK(rc == PFMSCAN_OK && n == (int64_t)wr.size());
        if (rc == PFMSCAN_OK && n == (int64_t)wr.size()) {
            CHECK(std::memcmp(f, wf.data(), wf.size() * sizeof(int64_t)) == 0);
            CHECK(wr.empty() || std::memcmp(g, wr.data(), wr.size() * sizeof(int64_t)) == 0);
            CHECK(wm.empty() || std::memcmp(k, wm.data(), wm.size() * sizeof(int64_t)) == 0);
        }
        std::free(f), std::free(g), std::free(k);
    }
    std::free(first0), std::free(hp), std::free(ho), std::free(hl), std::free(hm);
}

static void order_round(std::mt19937_64 &rng)
{
    const int n_motifs = (int)(rng() % 6), n = (int)(rng() % 40);
    std::vector<int64_t> pos((size_t)n);
    std::vector<int32_t> mot((size_t)n);
    bool ok = true;
    for (int h = 0; h < n; ++h) {
        pos[(size_t)h] = h / 2;
        mot[(size_t)h] = rng() % 17 == 0 ? (int32_t)(rng() % 9) - 2 : (n_motifs ? (int32_t)(rng() % (uint64_t)n_motifs) : 0);
        ok = ok && mot[(size_t)h] >= 0 && mot[(size_t)h] < n_motifs;
    }
    int64_t *hp = heap(pos), *o = room<int64_t>((size_t)n);
    int32_t *hm = heap(mot);
    const int rc = pfmscan_site_order_lib(hp, hm, n, n_motifs, o);
    CHECK(rc == (ok ? PFMSCAN_OK : PFMSCAN_E_BADARG));
    if (ok && rc == PFMSCAN_OK) {
        std::vector<int64_t> want((size_t)n);
        std::iota(want.begin(), want.end(), 0);
        std::stable_sort(want.begin(), want.end(), [&](int64_t a, int64_t b) { return mot[(size_t)a] < mot[(size_t)b]; });
        CHECK(n == 0 || std::memcmp(o, want.data(), (size_t)n * sizeof(int64_t)) == 0);
    }
    std::free(hp), std::free(hm), std::free(o);
}

static double from_bits(uint64_t b)
{
    double v;
    std::memcpy(&v, &b, sizeof(v));
    return v;
}

static void acc_round_trip(std::mt19937_64 &rng)
{
    const int L = PFMSCAN_SITE_LIMBS;
    // values of every exponent, subnormals included; a few zeros
    const int n = 1 + (int)(rng() % 24), cut = (int)(rng() % (uint64_t)(n + 1));
    std::vector<double> v((size_t)n);
    for (auto &x : v) x = rng() % 11 == 0 ? 0.0 : from_bits(((rng() % 2047) << 52) | (rng() & ((uint64_t(1) << 52) - 1)));
    double *hv = heap(v);
    uint64_t *whole = room<uint64_t>(L), *a = room<uint64_t>(L), *b = room<uint64_t>(L), *sum = room<uint64_t>(L), *norm = room<uint64_t>(L);
    CHECK(pfmscan_site_acc_from_doubles(hv, n, whole) == PFMSCAN_OK);
    CHECK(pfmscan_site_acc_from_doubles(hv, cut, a) == PFMSCAN_OK);
    CHECK(pfmscan_site_acc_from_doubles(hv + cut, n - cut, b) == PFMSCAN_OK);
    std::memset(sum, 0, L * sizeof(uint64_t));
    std::memset(norm, 0, L * sizeof(uint64_t));
    CHECK(pfmscan_site_acc_add(sum, a, 1, 1) == PFMSCAN_OK);
    for (int i = 0; i < L - 1; ++i) CHECK(sum[i] < (uint64_t(1) << 32));
    CHECK(pfmscan_site_acc_add(sum, b, 1, 1) == PFMSCAN_OK);
    CHECK(pfmscan_site_acc_add(norm, whole, 1, 1) == PFMSCAN_OK);
    for (int i = 0; i < L - 1; ++i) CHECK(sum[i] < (uint64_t(1) << 32));
    CHECK(std::memcmp(sum, norm, L * sizeof(uint64_t)) == 0);
    double r1 = -1, r2 = -1;
    CHECK(pfmscan_site_acc_round(whole, 1, 1, &r1) == PFMSCAN_OK && pfmscan_site_acc_round(norm, 1, 1, &r2) == PFMSCAN_OK);
    CHECK(std::memcmp(&r1, &r2, sizeof(r1)) == 0);
    // one value rounds back to itself; v + v is 2 v (+inf past DBL_MAX)
    double *two = room<double>(2), got = -1;
    two[0] = two[1] = v[0];
    CHECK(pfmscan_site_acc_from_doubles(two, 1, a) == PFMSCAN_OK && pfmscan_site_acc_round(a, 1, 1, &got) == PFMSCAN_OK);
    CHECK(got == v[0]);
    CHECK(pfmscan_site_acc_from_doubles(two, 2, a) == PFMSCAN_OK && pfmscan_site_acc_round(a, 1, 1, &got) == PFMSCAN_OK);
    CHECK(got == v[0] + v[0]);
    // what the decomposition must never see
    two[1] = rng() % 3 == 0 ? -1.0 : (rng() % 2 ? INFINITY : NAN);
    CHECK(pfmscan_site_acc_from_doubles(two, 2, a) == PFMSCAN_E_BADARG);
    std::free(hv), std::free(whole), std::free(a), std::free(b), std::free(sum), std::free(norm), std::free(two);
}

// several accumulators of several cells: the strides of add and round
static void acc_strides(std::mt19937_64 &rng)
{
    const int L = PFMSCAN_SITE_LIMBS, n_acc = 1 + (int)(rng() % 3), n_cells = 1 + (int)(rng() % 5);
    const size_t words = (size_t)n_acc * L * (size_t)n_cells;
    uint64_t *raw = room<uint64_t>(words), *dst = room<uint64_t>(words), *cell = room<uint64_t>(L);
    double *want = room<double>((size_t)n_acc * n_cells), *got = room<double>((size_t)n_acc * n_cells);
    std::memset(dst, 0, words * sizeof(uint64_t));
    for (int k = 0; k < n_acc; ++k)
        for (int e = 0; e < n_cells; ++e) {
            double v[3];
            for (auto &x : v) x = from_bits(((rng() % 2046) << 52) | (rng() & ((uint64_t(1) << 52) - 1)));
            CHECK(pfmscan_site_acc_from_doubles(v, 3, cell) == PFMSCAN_OK);
            CHECK(pfmscan_site_acc_round(cell, 1, 1, &want[k * n_cells + e]) == PFMSCAN_OK);
            for (int i = 0; i < L; ++i) raw[((size_t)k * L + i) * n_cells + e] = cell[i];
        }
    CHECK(pfmscan_site_acc_add(dst, raw, n_acc, n_cells) == PFMSCAN_OK);
    CHECK(pfmscan_site_acc_round(dst, n_acc, n_cells, got) == PFMSCAN_OK);
    CHECK(std::memcmp(want, got, (size_t)n_acc * n_cells * sizeof(double)) == 0);
    std::free(raw), std::free(dst), std::free(cell), std::free(want), std::free(got);
}

int main(int argc, char **argv)
{
    const int rounds = argc > 1 ? std::atoi(argv[1]) : 1000;
    std::mt19937_64 rng(4321);
    auto pick = [&](int64_t lo, int64_t hi) { return lo + (int64_t)(rng() % (uint64_t)(hi - lo + 1)); };
    const int64_t nasty[] = {0, -1, 1, INT64_MAX, INT64_MIN, INT64_MAX - 1, INT64_MIN + 1, (int64_t)1 << 62, -((int64_t)1 << 62), 4096, 4097};
    for (int it = 0; it < rounds; ++it) {
        const int m = (int)pick(1, 12), n_motifs = (int)pick(1, 5);
        std::vector<int64_t> off, len, pos;
        std::vector<int32_t> mot;
        int64_t at = pick(0, 3);
        const int n_rec = (int)pick(0, 8);
        for (int r = 0; r < n_rec; ++r) {
            const int64_t L = it % 50 == 0 && r == 1 ? pick(4090, 12400) : pick(0, 40);
            off.push_back(at);
            len.push_back(L);
            at += L + pick(1, 3);
        }
        // motif-major: each motif takes each window with some probability (none at all now and then: empty motifs)
        for (int k = 0; k < n_motifs; ++k) {
            const int dense = (it + k) % 4 == 0 ? 1 : (int)pick(2, 9);
            if (pick(0, 4) == 0) continue;
            for (int r = 0; r < n_rec; ++r)
                for (int64_t s = 0; s + m <= len[r]; ++s)
                    if (dense == 1 || pick(1, dense) == 1) {
                        pos.push_back(off[r] + s);
                        mot.push_back(k);
                    }
        }
        one(pos, mot, n_motifs, off, len, m);
        // ... then broken in one place
        std::vector<int64_t> p2 = pos, o2 = off, l2 = len;
        std::vector<int32_t> m2 = mot;
        switch (pick(0, 9)) {
        case 0: if (p2.size() > 1) { const size_t i = (size_t)pick(1, (int64_t)p2.size() - 1); p2[i] = p2[i - 1]; } break;
        case 1: if (p2.size() > 1) { const size_t i = (size_t)pick(1, (int64_t)p2.size() - 1); std::swap(p2[i], p2[i - 1]); } break;
        case 2: if (!p2.empty()) p2[(size_t)pick(0, (int64_t)p2.size() - 1)] += pick(1, 14); break;
        case 3: if (!p2.empty()) p2.back() = at + pick(0, 5); break;
        case 4: if (!o2.empty()) o2[(size_t)pick(0, (int64_t)o2.size() - 1)] = nasty[pick(0, 10)]; break;
        case 5: if (!l2.empty()) l2[(size_t)pick(0, (int64_t)l2.size() - 1)] = nasty[pick(0, 10)]; break;
        case 6: if (!p2.empty()) p2[(size_t)pick(0, (int64_t)p2.size() - 1)] = nasty[pick(0, 10)]; break;
        case 7: if (!m2.empty()) m2[(size_t)pick(0, (int64_t)m2.size() - 1)] = (int32_t)pick(-2, n_motifs + 1); break;
        case 8: if (m2.size() > 1) std::swap(m2.front(), m2.back()); break;
        default: if (o2.size() > 1) std::swap(o2[0], o2[1]); break;
        }
        one(p2, m2, n_motifs, o2, l2, m);
        order_round(rng);
        acc_round_trip(rng);
        acc_strides(rng);
    }
    // the top of the range: DBL_MAX twice is +inf, the largest subnormal and the smallest double come back
    const int L = PFMSCAN_SITE_LIMBS;
    uint64_t *acc = room<uint64_t>(L);
    double big[2] = {1.7976931348623157e308, 1.7976931348623157e308}, got = 0;
    CHECK(pfmscan_site_acc_from_doubles(big, 2, acc) == PFMSCAN_OK && pfmscan_site_acc_round(acc, 1, 1, &got) == PFMSCAN_OK && std::isinf(got));
    CHECK(pfmscan_site_acc_from_doubles(big, 1, acc) == PFMSCAN_OK && acc[L - 1] != 0 && pfmscan_site_acc_round(acc, 1, 1, &got) == PFMSCAN_OK && got == big[0]);
    double tiny[2] = {4.9406564584124654e-324, 2.2250738585072009e-308};
    CHECK(pfmscan_site_acc_from_doubles(tiny, 1, acc) == PFMSCAN_OK && acc[0] == 1 && pfmscan_site_acc_round(acc, 1, 1, &got) == PFMSCAN_OK && got == tiny[0]);
    CHECK(pfmscan_site_acc_from_doubles(tiny + 1, 1, acc) == PFMSCAN_OK && pfmscan_site_acc_round(acc, 1, 1, &got) == PFMSCAN_OK && got == tiny[1]);
    std::free(acc);
    // arguments that are refused outright
    int64_t n = 0, x = 0;
    int32_t k = 0;
    CHECK(pfmscan_site_groups_lib(nullptr, &k, 1, 1, &x, &x, 1, 3, 0, &x, &x, &x, &n) == PFMSCAN_E_BADARG);
    CHECK(pfmscan_site_groups_lib(&x, nullptr, 1, 1, &x, &x, 1, 3, 0, &x, &x, &x, &n) == PFMSCAN_E_BADARG);
    CHECK(pfmscan_site_groups_lib(&x, &k, 1, 1, &x, &x, 1, 0, 0, &x, &x, &x, &n) == PFMSCAN_E_BADARG);
    CHECK(pfmscan_site_groups_lib(&x, &k, 1, -1, &x, &x, 1, 3, 0, &x, &x, &x, &n) == PFMSCAN_E_BADARG);
    CHECK(pfmscan_site_groups_lib(&x, &k, 1, 1, &x, &x, 1, 3, 0, &x, &x, &x, nullptr) == PFMSCAN_E_BADARG);
    CHECK(pfmscan_site_order_lib(&x, &k, -1, 1, &x) == PFMSCAN_E_BADARG);
    CHECK(pfmscan_site_acc_add(nullptr, nullptr, 1, 1) == PFMSCAN_E_BADARG);
    CHECK(pfmscan_site_acc_round(nullptr, 1, 1, nullptr) == PFMSCAN_E_BADARG);
    CHECK(pfmscan_site_acc_from_doubles(nullptr, 1, nullptr) == PFMSCAN_E_BADARG);
    if (failures) return 1;
    std::printf("ok %d rounds\n", rounds);
    return 0;
}
