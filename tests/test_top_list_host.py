"""csrc/top_list.hpp: TopList<N, Ord>, the sorted register list behind the top-n selection kernels (kernel_topwords.hpp,
kernel_scored.hpp, kernel_ecdf.hpp, kernel_nearest.hpp).  Its constructor, admits, insert and fold_sorted are plain C++: they are
compiled here with the host compiler around a driver with two toy orders -- an unsigned key of two 32-bit words, ascending, and
(double descending by IEEE compare, id ascending) as one 64-bit and one 32-bit word, fed -0.0, +0.0, both infinities and repeated
scores: between them both kinds of word, alone and mixed -- and checked against a
sort of the input for every order of arrival of 7 entries and for seeded random sequences of 40, which the GPU tests reach only by
chance.  pop_wave needs a wavefront; the GPU tests of the four kernels cover it."""
import os
import subprocess

import pytest

from conftest import ROOT

N_RANDOM = 3000
DRIVER = r"""
#include "top_list.hpp"
#include <algorithm>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

struct KeyOrd {                                           // w[0] high, w[1] low word of a key; all ones is the padding
    static constexpr int Q = 0, W = 2;
    typedef TopEntry<0, 2> E;
    static uint64_t key(const E &e) { return ((uint64_t)e.w[0] << 32) | e.w[1]; }
    static E entry(uint32_t hi, uint32_t lo) { return E{{0}, {hi, lo}}; }
    E pad() const { return entry(0xFFFFFFFFu, 0xFFFFFFFFu); }
    bool before(const E &a, const E &b) const { return key(a) < key(b); }
    bool same(const E &a, const E &b) const { return key(a) == key(b); }
};

struct ScoreOrd {                                         // q[0] the double's bits, w[0] the id; (-inf, all ones) pads
    static constexpr int Q = 1, W = 1;
    typedef TopEntry<1, 1> E;
    static double score(const E &e) { double s; memcpy(&s, &e.q[0], 8); return s; }
    static E entry(double s, uint32_t id) { uint64_t b; memcpy(&b, &s, 8); return E{{b}, {id}}; }
    E pad() const { return entry(-INFINITY, 0xFFFFFFFFu); }
    bool before(const E &a, const E &b) const { return score(a) > score(b) || (score(a) == score(b) && a.w[0] < b.w[0]); }
    bool same(const E &a, const E &b) const { return a.w[0] == b.w[0]; }
};

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() { g_rng = g_rng * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(g_rng >> 33); }

// bits: a -0.0 stays one (an array the order does not use holds zeros)
template <class E> static bool equal(const E &a, const E &b) { return memcmp(a.q, b.q, sizeof a.q) == 0 && memcmp(a.w, b.w, sizeof a.w) == 0; }

static void fail(const char *what, int N, int Q) { fprintf(stderr, "FAIL: %s (N = %d, Q = %d)\n", what, N, Q); exit(1); }

// `in` in its order of arrival, `want` the same entries sorted by the order
template <int N, class Ord>
static void check(const std::vector<typename Ord::E> &in, const std::vector<typename Ord::E> &want)
{
    typedef typename Ord::E E;
    const Ord ord{};
    const int M = (int)in.size();
    TopList<N, Ord> L;
    for (const E &e : in) if (L.admits(e)) L.insert(e);
    for (int j = 0; j < N; ++j)
        if (!equal(L.at(j), j < M ? want[j] : ord.pad())) fail("the list is not the sorted prefix followed by the padding", N, Ord::Q);
    for (int j = N; j < M; ++j)
        if (L.admits(want[j])) fail("an entry outside the prefix is admitted", N, Ord::Q);
    if (L.admits(ord.pad())) fail("the padding is admitted", N, Ord::Q);
    // partial lists as the kernels leave them: a strided share of the input each, the first n places of a TopList<N>
    const int pieces = 1 + (int)(rnd() % 5), shift = (int)(rnd() % 5);
    const int ns[2] = {N, (N + 1) / 2};
    for (int n : ns) {
        TopList<N, Ord> F;
        for (int p = 0; p < pieces; ++p) {
            TopList<N, Ord> P;
            for (int i = 0; i < M; ++i) if ((i + shift) % pieces == p && P.admits(in[i])) P.insert(in[i]);
            std::vector<E> part;
            for (int j = 0; j < n; ++j) part.push_back(P.at(j));
            F.fold_sorted(n, [&](int j) { return part[j]; });
        }
        for (int j = 0; j < n; ++j)
            if (!equal(F.at(j), j < M ? want[j] : ord.pad())) fail("fold_sorted over partial lists differs from inserting everything", N, Ord::Q);
    }
}

template <class Ord>
static void check_all(const std::vector<typename Ord::E> &in, const std::vector<typename Ord::E> &want)
{
    check<1, Ord>(in, want); check<2, Ord>(in, want); check<4, Ord>(in, want); check<10, Ord>(in, want); check<16, Ord>(in, want);
}

static bool key_less(const KeyOrd::E &a, const KeyOrd::E &b) { return KeyOrd::key(a) < KeyOrd::key(b); }
static bool score_less(const ScoreOrd::E &a, const ScoreOrd::E &b)
{
    const double s = ScoreOrd::score(a), t = ScoreOrd::score(b);
    if (s != t) return s > t;                             // (-0.0 == +0.0: the id decides)
    return a.w[0] < b.w[0];
}

template <class Ord, class Less>
static long run(std::vector<typename Ord::E> seven, const std::vector<typename Ord::E> &palette_of_forty, int n_random, Less less)
{
    long cases = 0;
    std::vector<typename Ord::E> want = seven;
    std::sort(want.begin(), want.end(), less);
    std::vector<int> perm = {0, 1, 2, 3, 4, 5, 6};
    do {
        std::vector<typename Ord::E> in;
        for (int i : perm) in.push_back(seven[i]);
        check_all<Ord>(in, want);
        ++cases;
    } while (std::next_permutation(perm.begin(), perm.end()));
    for (int t = 0; t < n_random; ++t) {
        std::vector<typename Ord::E> in = palette_of_forty;
        for (int i = 39; i > 0; --i) std::swap(in[i], in[rnd() % (i + 1)]);
        if (Ord::Q == 0) for (auto &e : in) e.w[0] = rnd() % 5;             // ties in the high word; the low word is unique
        else for (auto &e : in) e.w[0] = (e.w[0] * 7 + (uint32_t)t) % 40;    // another id for the same score (7 is a unit mod 40)
        want = in;
        std::sort(want.begin(), want.end(), less);
        check_all<Ord>(in, want);
        ++cases;
    }
    return cases;
}

int main(int argc, char **argv)
{
    const int n_random = atoi(argv[1]);
    const uint32_t hl[7][2] = {{0, 0}, {0, 1}, {1, 0}, {0x7FFFFFFFu, 5}, {0x80000000u, 4}, {0xFFFFFFFFu, 0xFFFFFFFEu}, {0xFFFFFFFEu, 0xFFFFFFFFu}};
    std::vector<KeyOrd::E> k7, k40;
    for (int i = 0; i < 7; ++i) k7.push_back(KeyOrd::entry(hl[i][0], hl[i][1]));
    for (uint32_t i = 0; i < 40; ++i) k40.push_back(KeyOrd::entry(0, i));
    printf("key %ld\n", run<KeyOrd>(k7, k40, n_random, key_less));
    const double s7[7] = {-0.0, 0.0, INFINITY, -INFINITY, 1.5, 1.5, -INFINITY};
    const double s8[8] = {-INFINITY, -1.0, -0.0, 0.0, 0.5, 1.5, 1.5, INFINITY};
    std::vector<ScoreOrd::E> e7, e40;
    for (uint32_t i = 0; i < 7; ++i) e7.push_back(ScoreOrd::entry(s7[i], 6 - i));
    for (uint32_t i = 0; i < 40; ++i) e40.push_back(ScoreOrd::entry(s8[i % 8], i));
    printf("score %ld\n", run<ScoreOrd>(e7, e40, n_random, score_less));
    return 0;
}
"""


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("top_list")
    src, exe = d / "driver.cpp", str(d / "driver")
    src.write_text(DRIVER)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe, str(src), "-I", os.path.join(ROOT, "lda_thesis_amd", "csrc")])
    return exe


def test_every_arrival_order_gives_the_sorted_prefix(driver):
    """Every permutation of 7 entries and N_RANDOM shuffled sequences of 40, for N in {1, 2, 4, 10, 16} and both orders: the list is
    the first N of the sorted input then the padding, admits() refuses every other entry, and fold_sorted over the sorted partial
    lists of a split (all N places, or the first half of them) gives what inserting everything gives.  The driver exits non-zero at
    the first difference."""
    out = subprocess.run([driver, str(N_RANDOM)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    assert out.returncode == 0, out.stderr
    assert out.stdout.split() == ["key", str(5040 + N_RANDOM), "score", str(5040 + N_RANDOM)]
