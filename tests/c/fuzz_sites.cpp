// fuzz_sites.cpp -- pfmscan_site_groups (rnascan_amd/csrc/pfmscan_sites_host.hip, host only) under the sanitizers: random
// and adversarial record tables and hit lists in exact-size heap buffers, every accepted answer checked against the
// definition (include/pfmscan.h).  Built and run by tests/test_sites_cpu.py with g++ -fsanitize=address,undefined.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
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
static int64_t *heap(const std::vector<int64_t> &v)
{
    int64_t *p = static_cast<int64_t *>(std::malloc(v.size() ? v.size() * sizeof(int64_t) : 1));
    if (!v.empty()) std::memcpy(p, v.data(), v.size() * sizeof(int64_t));
    return p;
}

// the definition, plainly: is the input valid, and which record holds each hit
static bool valid(const std::vector<int64_t> &pos, const std::vector<int64_t> &off, const std::vector<int64_t> &len, int m,
                  std::vector<int64_t> &rec)
{
    for (size_t r = 0; r < off.size(); ++r) {
        if (off[r] < 0 || len[r] < 0 || len[r] > INT64_MAX - off[r]) return false;
        if (r > 0 && off[r] <= off[r - 1] + len[r - 1]) return false;
    }
    rec.clear();
    for (size_t h = 0; h < pos.size(); ++h) {
        if (h > 0 && pos[h] <= pos[h - 1]) return false;
        int64_t found = -1;
        for (size_t r = 0; r < off.size(); ++r)
            if (pos[h] >= off[r] && pos[h] < off[r] + len[r] && m <= off[r] + len[r] - pos[h]) found = (int64_t)r;
        if (found < 0) return false;
        rec.push_back(found);
    }
    return true;
}

static void one(const std::vector<int64_t> &pos, const std::vector<int64_t> &off, const std::vector<int64_t> &len, int m)
{
    std::vector<int64_t> rec;
    const bool ok = valid(pos, off, len, m, rec);
    int64_t *hp = heap(pos), *ho = heap(off), *hl = heap(len);
    const int64_t n_hits = (int64_t)pos.size(), n_rec = (int64_t)off.size();
    // capacity protocol: 0 first
    int64_t n = -7;
    int64_t *first0 = static_cast<int64_t *>(std::malloc(sizeof(int64_t)));
    int rc = pfmscan_site_groups(hp, n_hits, ho, hl, n_rec, m, 0, first0, nullptr, &n);
    if (!ok) {
        CHECK(rc == PFMSCAN_E_BADARG);
    } else {
        // the groups by the definition: runs of one record, cut every PFMSCAN_SITE_GROUP hits
        std::vector<int64_t> wf, wr;
        for (int64_t h = 0, run = 0; h < n_hits; ++h) {
            if (h == 0 || rec[h] != rec[h - 1] || run == PFMSCAN_SITE_GROUP) {
                wf.push_back(h);
                wr.push_back(rec[h]);
                run = 0;
            }
            ++run;
        }
        wf.push_back(n_hits);
        CHECK(n == (int64_t)wr.size());
        CHECK(rc == (wr.empty() ? PFMSCAN_OK : PFMSCAN_E_CAPACITY));
        if (!wr.empty()) {                                  // one short: still refused, nothing written
            int64_t *f = static_cast<int64_t *>(std::malloc(wr.size() * sizeof(int64_t)));
            int64_t *g = static_cast<int64_t *>(std::malloc(wr.size() > 1 ? (wr.size() - 1) * sizeof(int64_t) : 1));
            CHECK(pfmscan_site_groups(hp, n_hits, ho, hl, n_rec, m, (int64_t)wr.size() - 1, f, g, &n) == PFMSCAN_E_CAPACITY);
            CHECK(n == (int64_t)wr.size());
            std::free(f);
            std::free(g);
        }
        int64_t *f = static_cast<int64_t *>(std::malloc((wr.size() + 1) * sizeof(int64_t)));
        int64_t *g = static_cast<int64_t *>(std::malloc(wr.empty() ? 1 : wr.size() * sizeof(int64_t)));
        rc = pfmscan_site_groups(hp, n_hits, ho, hl, n_rec, m, (int64_t)wr.size(), f, g, &n);
        CHECK(rc == PFMSCAN_OK && n == (int64_t)wr.size());
        if (rc == PFMSCAN_OK && n == (int64_t)wr.size()) {
            CHECK(std::memcmp(f, wf.data(), wf.size() * sizeof(int64_t)) == 0);
            CHECK(wr.empty() || std::memcmp(g, wr.data(), wr.size() * sizeof(int64_t)) == 0);
        }
        std::free(f);
        std::free(g);
    }
    std::free(first0);
    std::free(hp);
    std::free(ho);
    std::free(hl);
}

int main(int argc, char **argv)
{
    const int rounds = argc > 1 ? std::atoi(argv[1]) : 1000;
    std::mt19937_64 rng(12345);
    auto pick = [&](int64_t lo, int64_t hi) { return lo + (int64_t)(rng() % (uint64_t)(hi - lo + 1)); };
    const int64_t nasty[] = {0, -1, 1, INT64_MAX, INT64_MIN, INT64_MAX - 1, INT64_MIN + 1, (int64_t)1 << 62, -((int64_t)1 << 62), 4096, 4097};
    for (int it = 0; it < rounds; ++it) {
        const int m = (int)pick(1, 12);
        // a well-formed table ...
        std::vector<int64_t> off, len, pos;
        int64_t at = pick(0, 3);
        const int n_rec = (int)pick(0, 8);
        for (int r = 0; r < n_rec; ++r) {
            const int64_t L = it % 50 == 0 && r == 1 ? pick(4090, 12400) : pick(0, 40);
            off.push_back(at);
            len.push_back(L);
            at += L + pick(1, 3);
        }
        // ... and hits inside it: each window with some probability (all of them every fourth round)
        const int dense = it % 4 == 0 ? 1 : (int)pick(2, 9);
        for (int r = 0; r < n_rec; ++r)
            for (int64_t s = 0; s + m <= len[r]; ++s)
                if (dense == 1 || pick(1, dense) == 1) pos.push_back(off[r] + s);
        one(pos, off, len, m);
        // ... then broken in one place
        std::vector<int64_t> p2 = pos, o2 = off, l2 = len;
        switch (pick(0, 7)) {
        case 0: if (p2.size() > 1) { const size_t i = (size_t)pick(1, (int64_t)p2.size() - 1); p2[i] = p2[i - 1]; } break;
        case 1: if (p2.size() > 1) { const size_t i = (size_t)pick(1, (int64_t)p2.size() - 1); std::swap(p2[i], p2[i - 1]); } break;
        case 2: if (!p2.empty()) p2[(size_t)pick(0, (int64_t)p2.size() - 1)] += pick(1, 14); break;          // maybe across a separator
        case 3: if (!p2.empty()) p2.back() = at + pick(0, 5); break;                                         // past the stream
        case 4: if (!o2.empty()) o2[(size_t)pick(0, (int64_t)o2.size() - 1)] = nasty[pick(0, 10)]; break;
        case 5: if (!l2.empty()) l2[(size_t)pick(0, (int64_t)l2.size() - 1)] = nasty[pick(0, 10)]; break;
        case 6: if (!p2.empty()) p2[(size_t)pick(0, (int64_t)p2.size() - 1)] = nasty[pick(0, 10)]; break;
        default: if (o2.size() > 1) std::swap(o2[0], o2[1]); break;
        }
        one(p2, o2, l2, m);
    }
    // arguments that are refused outright
    int64_t n = 0, x = 0;
    CHECK(pfmscan_site_groups(nullptr, 1, &x, &x, 1, 3, 0, &x, &x, &n) == PFMSCAN_E_BADARG);
    CHECK(pfmscan_site_groups(&x, 1, &x, &x, 1, 0, 0, &x, &x, &n) == PFMSCAN_E_BADARG);
    CHECK(pfmscan_site_groups(&x, 1, &x, &x, 1, PFMSCAN_MAX_WIDTH + 1, 0, &x, &x, &n) == PFMSCAN_E_BADARG);
    CHECK(pfmscan_site_groups(&x, -1, &x, &x, 1, 3, 0, &x, &x, &n) == PFMSCAN_E_BADARG);
    CHECK(pfmscan_site_groups(&x, 1, &x, &x, 1, 3, 0, &x, &x, nullptr) == PFMSCAN_E_BADARG);
    if (failures) return 1;
    std::printf("ok %d rounds\n", rounds);
    return 0;
}
