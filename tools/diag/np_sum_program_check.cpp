// Stand-alone host check of numpy's float32 np.sum as a program (pw_build / pw_eval,
// csrc/loudness.h): every index of a built program lies inside its tables, the
// program stays within the limits the device kernel is sized for, and pw_eval
// equals, bit for bit, a plain recursion of numpy's pairwise sum written out below.
// No context, no GPU, never loaded into Python.  Only the host part of the header
// is compiled (no HIP); build it instrumented and run it on the CPU:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer \
//     -ffp-contract=off tools/diag/np_sum_program_check.cpp -o np_sum_program_check
// Exits non-zero on any failure.
#include <cstdio>
#include <cstring>

#define MM_LOUDNESS_HOST_ONLY
#include "../../python-audio-mastering_amd/csrc/loudness.h"

static int failures = 0;

#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) {                                                           \
            fprintf(stderr, "line %d, n = %lld: %s failed\n", __LINE__, cur_n, #cond); \
            ++failures;                                                          \
        }                                                                        \
    } while (0)
static long long cur_n = 0;

// numpy's pairwise sum of m contiguous float32 values (pairwise_sum_FLOAT)
static float np_pairwise(const float *a, int64_t m) {
    if (m < 8) {
        float res = 0.0f;  // (0 + a[0] is a[0] bit for bit: the inputs are squares, never -0)
        for (int64_t i = 0; i < m; ++i) res += a[i];
        return res;
    }
    if (m <= 128) {
        float r[8];
        for (int q = 0; q < 8; ++q) r[q] = a[q];
        int64_t i = 8;
        for (; i < m - m % 8; i += 8)
            for (int q = 0; q < 8; ++q) r[q] += a[i + q];
        float res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
        for (; i < m; ++i) res += a[i];
        return res;
    }
    int64_t n2 = m / 2;
    n2 -= n2 % 8;
    return np_pairwise(a, n2) + np_pairwise(a + n2, m - n2);
}

// np.sum over n contiguous float32 values: 8192-element buffers summed in order
static float np_sum(const float *a, int64_t n) {
    float res = 0.0f;
    for (int64_t o = 0; o < n; o += 8192) res += np_pairwise(a + o, std::min<int64_t>(8192, n - o));
    return res;
}

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint32_t rng() {  // xorshift64*
    rng_state ^= rng_state >> 12;
    rng_state ^= rng_state << 25;
    rng_state ^= rng_state >> 27;
    return (uint32_t)((rng_state * 0x2545f4914f6cdd1dull) >> 32);
}

static void run(int64_t n) {
    cur_n = (long long)n;
    std::vector<int32_t> P;
    pw_build(n, P);
    CHECK(P.size() >= 5);
    if (P.size() < 5) return;
    const int64_t nl = P[0], nn = P[1], nlev = P[2], nch = P[3], root = P[4];
    CHECK(nl >= 0 && nn >= 0 && nlev >= 0 && nch == (n + KB_CHUNK - 1) / KB_CHUNK);
    // the layout gate.hip reads: chunk_leaf[nch + 1], leaf_off[nl], leaf_len[nl], node_a[nn], node_b[nn], level_node[nlev + 1]
    const int64_t want = 5 + (nch + 1) + 2 * nl + 2 * nn + (nlev + 1);
    CHECK((int64_t)P.size() == want);
    if ((int64_t)P.size() != want) return;
    const int32_t *chunk_leaf = P.data() + 5, *loff = chunk_leaf + nch + 1, *llen = loff + nl, *na = llen + nl,
                  *nb = na + nn, *lvl = nb + nn;
    if (n <= 76800) {  // every block length up to 0.4 s at 192 kHz fits the kernel's LDS tables
        CHECK(nl + nn <= KB_VMAX);
        CHECK((int64_t)P.size() <= KB_PMAX);
    }
    CHECK(n == 0 ? root == -1 : (root >= 0 && root < nl + nn));
    // chunks: ascending leaf ranges covering every leaf; a chunk's leaves lie inside it
    CHECK(chunk_leaf[0] == 0 && chunk_leaf[nch] == nl);
    int64_t next = 0;  // the leaves tile [0, n) in order
    for (int64_t c = 0; c < nch; ++c) {
        CHECK(chunk_leaf[c] < chunk_leaf[c + 1]);
        for (int64_t li = chunk_leaf[c]; li < chunk_leaf[c + 1] && li < nl; ++li) {
            CHECK(loff[li] == next && llen[li] >= 1 && llen[li] <= 128);
            CHECK(loff[li] >= c * KB_CHUNK && loff[li] + llen[li] <= std::min<int64_t>((c + 1) * KB_CHUNK, n));
            next = (int64_t)loff[li] + llen[li];
        }
    }
    CHECK(next == n);
    // levels: ascending node ranges covering every node; a node reads leaves or nodes of lower levels
    CHECK(lvl[0] == 0 && lvl[nlev] == nn);
    for (int64_t L = 0; L < nlev; ++L) {
        CHECK(lvl[L] <= lvl[L + 1]);
        for (int64_t k = lvl[L]; k < lvl[L + 1] && k < nn; ++k) {
            CHECK(na[k] >= 0 && na[k] < nl + lvl[L]);
            CHECK(nb[k] >= 0 && nb[k] < nl + lvl[L]);
        }
    }
    if (failures) return;  // (pw_eval trusts the indices checked above)
    // squares of values in [0, 1): what the block sums add; every addition rounds
    std::vector<float> x((size_t)n + 1);
    for (auto &v : x) {
        const float u = (float)(rng() >> 8) * (1.0f / 16777216.0f);
        v = u * u;
    }
    const float got = pw_eval(P.data(), x.data()), ref = np_sum(x.data(), n);
    CHECK(memcmp(&got, &ref, sizeof got) == 0);
}

int main() {
    const int64_t fixed[] = {0, 1, 7, 8, 9, 127, 128, 129, 8191, 8192, 8193, 17640, 76800, 16 * (int64_t)KB_CHUNK};
    for (int64_t n : fixed) run(n);
    for (int i = 0; i < 300; ++i) run(1 + rng() % 76800);                      // block lengths the chain meets
    for (int i = 0; i < 60; ++i) run(76801 + rng() % (16 * KB_CHUNK - 76801));  // up to mm_np_sum_f32's limit
    printf("np_sum_program_check: %d failure(s)\n", failures);
    return failures ? 1 : 0;
}
