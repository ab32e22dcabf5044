// lookup_cpu.cpp -- a single-threaded CPU comparator for tools/lookup_probe.py.  It RESTATES the
// sequential algorithm of a halo2-style prover's permute_expression_pair in plain C++ (a comparison
// sort of the input, an ordered map value -> count of the table, the leftovers popped onto the
// repeated rows from the back); it is not the prover's Rust and shares no code with it.  Elements are
// 256-bit standard-form integers compared from the top limb down.
//
//   g++ -O2 -std=c++17 tools/lookup_cpu.cpp -o tools/lookup_cpu && tools/lookup_cpu 16 20 22
//
// For each log2 size and each kind of column (full: full-width random, the input drawing rows of the
// table; range16: a 16-bit range table padded with zeros, random 16-bit inputs) it prints the
// median of 3 runs of the sort alone and of the whole permuted pair, in milliseconds.
#include <algorithm>
#include <array>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <vector>

using El = std::array<uint64_t, 4>;
struct Less {
    bool operator()(const El& a, const El& b) const {
        for (int i = 3; i >= 0; --i)
            if (a[i] != b[i]) return a[i] < b[i];
        return false;
    }
};

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t next_u64() {  // splitmix64
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

static double now_ms() {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// returns the number of distinct input values the table lacks
static size_t permute_pair(const std::vector<El>& input, const std::vector<El>& table, std::vector<El>& a,
                           std::vector<El>& s) {
    a = input;
    std::sort(a.begin(), a.end(), Less());
    std::map<El, uint32_t, Less> left;
    for (const El& v : table) ++left[v];
    s.assign(a.size(), El{});
    std::vector<size_t> repeated;
    size_t missing = 0;
    for (size_t row = 0; row < a.size(); ++row) {
        if (row == 0 || a[row] != a[row - 1]) {
            s[row] = a[row];
            auto it = left.find(a[row]);
            if (it != left.end() && it->second) --it->second;
            else ++missing;
        } else {
            repeated.push_back(row);
        }
    }
    for (const auto& kv : left)
        for (uint32_t c = 0; c < kv.second && !repeated.empty(); ++c) {
            s[repeated.back()] = kv.first;
            repeated.pop_back();
        }
    return missing;
}

int main(int argc, char** argv) {
    for (int arg = 1; arg < argc; ++arg) {
        const int logn = atoi(argv[arg]);
        if (logn < 1 || logn > 26) continue;
        const size_t n = (size_t)1 << logn;
        for (int kind = 0; kind < 2; ++kind) {
            std::vector<El> table(n), input(n), a, s;
            for (size_t i = 0; i < n; ++i) {
                if (kind == 0) table[i] = {next_u64(), next_u64(), next_u64(), next_u64() >> 2};
                else table[i] = {i < 65536 ? i : 0, 0, 0, 0};
            }
            for (size_t i = 0; i < n; ++i) {
                if (kind == 0) input[i] = table[next_u64() % n];
                else input[i] = {next_u64() & 0xFFFF, 0, 0, 0};
            }
            double sort_ms[3], pair_ms[3];
            size_t missing = 0;
            for (int rep = 0; rep < 3; ++rep) {
                double t0 = now_ms();
                a = input;
                std::sort(a.begin(), a.end(), Less());
                sort_ms[rep] = now_ms() - t0;
                t0 = now_ms();
                missing = permute_pair(input, table, a, s);
                pair_ms[rep] = now_ms() - t0;
            }
            std::sort(sort_ms, sort_ms + 3);
            std::sort(pair_ms, pair_ms + 3);
            printf("cpu 2^%d %s: sort median %.1f ms, permuted pair median %.1f ms (missing %zu, check %llu)\n", logn,
                   kind == 0 ? "full" : "range16", sort_ms[1], pair_ms[1], missing, (unsigned long long)(s[n / 2][0] ^ a[n - 1][0]));
            fflush(stdout);
        }
    }
    return 0;
}
