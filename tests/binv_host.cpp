// Host harness for csrc/mbls_binv.hpp (the device inversion's algorithm, compiled here with g++):
// reads lines "<words> <hex word 0> ... <hex word words-1>" (12 = Fq modulus p, 8 = Fr modulus r),
// prints "<outer steps> <1 if the four-lane form (inverse_roles) agrees> <inverse words...>".  Driven by tests/test_oracle.py::test_binary_gcd_inverse.
//
// Trace mode (`binv_host trace`, same input): the same line followed by one token per sign
// correction, "a<k>" / "b<k>": lincomb_shift returned true for a (row f0, g0) or b (row f1, g1) in
// outer step k (1-based).  The outer loop is rebuilt here from the header's own primitives, the
// way inverse_roles is, and its steps and value must equal binv::inverse's (abort otherwise).
// Search mode (`binv_host search <words> <seed> <count>`): `count` values below the modulus from a
// splitmix64 stream; prints "<hex y> <outer steps> <corrections...>" for those with a correction.
// Driven by tests/golden/gen_binv_signs.py and tests/test_binv_model.py.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "mbls_binv.hpp"

static const uint32_t P[12] = {0xffffaaabu, 0xb9feffffu, 0xb153ffffu, 0x1eabfffeu, 0xf6b0f624u, 0x6730d2a0u,
                               0xf38512bfu, 0x64774b84u, 0x434bacd7u, 0x4b1ba7b6u, 0x397fe69au, 0x1a0111eau};
static const uint32_t R[8] = {0x00000001u, 0xffffffffu, 0xfffe5bfeu, 0x53bda402u,
                              0x09a1d805u, 0x3339d808u, 0x299d7d48u, 0x73eda753u};

struct Trace {
    int n = 0;
    int step[64];
    char row[64];
    void add(char r, int s) {
        if (n < 64) {
            row[n] = r;
            step[n++] = s;
        }
    }
};

// binv::inverse's outer loop from its primitives, recording where lincomb_shift returns true
template <int N>
static int inverse_traced(uint32_t (&out)[N], const uint32_t (&y)[N], const uint32_t (&m)[N], uint32_t ninv, Trace& tr) {
    using namespace mbls::binv;
    uint32_t a[N], b[N], u[N], v[N];
    for (int i = 0; i < N; ++i) {
        a[i] = y[i];
        b[i] = m[i];
        u[i] = i == 0 ? 1u : 0u;
        v[i] = 0;
    }
    int64_t pf0 = (int64_t)1 << K, pg0 = 0, pf1 = 0, pg1 = (int64_t)1 << K;
    int steps = 0;
    const int cap = (64 * N) / K + 8;
    while (!is_zero<N>(a) && steps < cap) {
        ++steps;
        const int nl = bitlen_or<N>(a, b);
        const int n = nl > 64 ? nl : 64;
        uint64_t xa = (a[0] & 0x7fffffffu) | (top33<N>(a, n - 33) << 31);
        uint64_t xb = (b[0] & 0x7fffffffu) | (top33<N>(b, n - 33) << 31);
        uint64_t F0 = 1, F1 = 1ull << 32;
        for (int j = 0; j < K; ++j) {
            const bool odd = (xa & 1) != 0;
            const bool lt = xa < xb;
            const bool sw = odd && lt;
            const uint64_t d = lt ? xb - xa : xa - xb;
            const uint64_t G0 = sw ? F1 : F0, G1 = sw ? F0 : F1;
            xb = sw ? xa : xb;
            xa = (odd ? d : xa) >> 1;
            F0 = odd ? G0 - G1 : G0;
            F1 = G1 << 1;
        }
        uint32_t nu[N], nv[N], na[N], nb[N];
        lincomb_mod<N>(nu, u, v, pf0, pg0, m, ninv);
        lincomb_mod<N>(nv, u, v, pf1, pg1, m, ninv);
        int64_t f0 = (int32_t)(uint32_t)F0, g0 = ((int64_t)F0 - f0) >> 32;
        int64_t f1 = (int32_t)(uint32_t)F1, g1 = ((int64_t)F1 - f1) >> 32;
        if (lincomb_shift<N>(na, a, b, f0, g0)) {
            tr.add('a', steps);
            f0 = -f0;
            g0 = -g0;
        }
        if (lincomb_shift<N>(nb, a, b, f1, g1)) {
            tr.add('b', steps);
            f1 = -f1;
            g1 = -g1;
        }
        for (int i = 0; i < N; ++i) {
            a[i] = na[i];
            b[i] = nb[i];
            u[i] = nu[i];
            v[i] = nv[i];
        }
        pf0 = f0;
        pg0 = g0;
        pf1 = f1;
        pg1 = g1;
    }
    lincomb_mod<N>(out, u, v, pf1, pg1, m, ninv);
    return steps;
}

template <int N>
static int traced_checked(uint32_t (&o)[N], const uint32_t (&y)[N], const uint32_t (&m)[N], uint32_t ninv, Trace& tr) {
    uint32_t t[N];
    const int steps = mbls::binv::inverse<N>(o, y, m, ninv);
    const int tsteps = inverse_traced<N>(t, y, m, ninv, tr);
    bool same = tsteps == steps;
    for (int i = 0; i < N; ++i) same = same && t[i] == o[i];
    if (!same) {
        fprintf(stderr, "binv_host: the traced loop disagrees with binv::inverse\n");
        abort();
    }
    return steps;
}

template <int N>
static void run(char* s, const uint32_t (&m)[N], uint32_t ninv, bool trace) {
    uint32_t y[N], o[N];
    for (int i = 0; i < N; ++i) y[i] = (uint32_t)strtoul(s, &s, 16);
    Trace tr;
    const int steps = trace ? traced_checked<N>(o, y, m, ninv, tr) : mbls::binv::inverse<N>(o, y, m, ninv);
    uint32_t q[N];
    const int qsteps = mbls::binv::inverse_roles<N>(q, y, m, ninv);  // the four-lane form, roles in turn
    bool same = qsteps == steps;
    for (int i = 0; i < N; ++i) same = same && q[i] == o[i];
    printf("%d %d", steps, same ? 1 : 0);
    for (int i = 0; i < N; ++i) printf(" %08x", o[i]);
    for (int i = 0; i < tr.n; ++i) printf(" %c%d", tr.row[i], tr.step[i]);
    printf("\n");
}

static uint64_t splitmix64(uint64_t& s) {
    uint64_t z = (s += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

template <int N>
static void search(const uint32_t (&m)[N], uint32_t ninv, uint64_t seed, long count) {
    const uint32_t topmask = 0xffffffffu >> __builtin_clz(m[N - 1]);
    for (long c = 0; c < count;) {
        uint32_t y[N], o[N];
        for (int i = 0; i < N; i += 2) {
            const uint64_t w = splitmix64(seed);
            y[i] = (uint32_t)w;
            y[i + 1] = (uint32_t)(w >> 32);
        }
        y[N - 1] &= topmask;
        bool lt = false, zero = true;  // 1 <= y < m, by rejection
        for (int i = N - 1; i >= 0; --i) {
            if (y[i] != m[i]) {
                lt = y[i] < m[i];
                break;
            }
        }
        for (int i = 0; i < N; ++i) zero = zero && y[i] == 0;
        if (!lt || zero) continue;
        ++c;
        Trace tr;
        const int steps = traced_checked<N>(o, y, m, ninv, tr);
        if (!tr.n) continue;
        for (int i = N - 1; i >= 0; --i) printf("%08x", y[i]);
        printf(" %d", steps);
        for (int i = 0; i < tr.n; ++i) printf(" %c%d", tr.row[i], tr.step[i]);
        printf("\n");
    }
}

int main(int argc, char** argv) {
    if (argc == 5 && !strcmp(argv[1], "search")) {
        const uint64_t seed = strtoull(argv[3], nullptr, 0);
        const long count = strtol(argv[4], nullptr, 0);
        if (atoi(argv[2]) == 12)
            search<12>(P, 0xfffcfffdu, seed, count);
        else
            search<8>(R, 0xffffffffu, seed, count);
        return 0;
    }
    const bool trace = argc == 2 && !strcmp(argv[1], "trace");
    char buf[1024];
    while (fgets(buf, sizeof buf, stdin)) {
        char* s = buf;
        const long words = strtol(s, &s, 10);
        if (words == 12)
            run<12>(s, P, 0xfffcfffdu, trace);
        else
            run<8>(s, R, 0xffffffffu, trace);
    }
    return 0;
}
