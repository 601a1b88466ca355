"""Host build of `csrc/unionfind.h` for the CPU tests: the header the kernels of graph.hip, tail.hip, linkage.hip and families.hip
include, compiled with a plain host C++ compiler into a stand-alone EXECUTABLE in which eight real threads race the header's
functions the way the kernels do -- unions from every thread, then the roots pass that stores roots into parent[] while other
threads still walk it -- and the result is compared with a sequential union-find written in the program itself.  Built with
`-fsanitize=thread` the program also fails on any access the sanitizer calls a race.  Nothing is loaded into Python: the test
runs the program as a child process.  Compiler discovery as in tests/hostbuild.py."""
import os
import subprocess

from tests.hostbuild import CSRC, _compiler

GRAPHS = ["chain_down", "chain_up", "star_hub_first", "star_hub_last", "two_chains", "random", "one_node", "two_nodes"]
TSAN = ("-O1", "-fsanitize=thread")
PLAIN = ("-O2",)

SOURCE = r"""
#include <stdint.h>
#include <stdio.h>
#include <atomic>
#include <thread>
#include <utility>
#include <vector>
#include "unionfind.h"

namespace {

constexpr int kThreads = 8;
typedef std::vector<std::pair<int32_t, int32_t>> Edges;

// the witness: one thread, plain memory, nothing of the header's
int32_t seq_find(std::vector<int32_t>& parent, int32_t x) {
    while (parent[x] != x) x = parent[x] = parent[parent[x]];
    return x;
}
std::vector<int32_t> expected(int32_t n, const Edges& edges) {
    std::vector<int32_t> parent(n), root(n);
    for (int32_t i = 0; i < n; ++i) parent[i] = i;
    for (const auto& e : edges) {
        const int32_t a = seq_find(parent, e.first), b = seq_find(parent, e.second);
        if (a != b) parent[a > b ? a : b] = a > b ? b : a;
    }
    for (int32_t i = 0; i < n; ++i) root[i] = seq_find(parent, i);
    return root;
}

// kThreads threads run body(t), released together
template <class F>
void race(F body) {
    std::atomic<int> waiting(kThreads);
    std::vector<std::thread> threads;
    for (int t = 0; t < kThreads; ++t)
        threads.emplace_back([&, t] {
            waiting.fetch_sub(1);
            while (waiting.load() > 0) std::this_thread::yield();
            body(t);
        });
    for (auto& th : threads) th.join();
}

int mismatches(const char* name, const char* what, const int32_t* got, const std::vector<int32_t>& want) {
    int bad = 0;
    for (size_t i = 0; i < want.size(); ++i)
        if (got[i] != want[i] && bad++ < 5) fprintf(stderr, "%s, %s: node %zu -> %d, expected %d\n", name, what, i, got[i], want[i]);
    return bad;
}

int run(const char* name, int32_t n, const Edges& edges) {
    const std::vector<int32_t> want = expected(n, edges);
    for (int32_t i = 0; i < n; ++i)
        if (want[i] > i) return fprintf(stderr, "%s: the witness names a root above node %d\n", name, i), 1;
    std::vector<int32_t> store(n), plain(n);
    int32_t* parent = store.data();
    for (int32_t i = 0; i < n; ++i) parent[i] = i;
    const size_t m = edges.size();
    // 1. the unions, edges dealt round-robin
    race([&](int t) {
        for (size_t k = t; k < m; k += kThreads) fal::uf_union<fal::kUfAgent>(parent, edges[k].first, edges[k].second);
    });
    // the plain-load find of a pass in which nothing writes parent[] (fam_find_kernel): one thread
    for (int32_t i = 0; i < n; ++i) plain[i] = fal::uf_find_final<fal::kUfPlainLoads>(parent, i);
    int bad = mismatches(name, "plain-load final find", plain.data(), want);
    // 2. the roots pass (dbscan_roots_kernel, lk_roots_kernel): rows dealt round-robin, every root stored while others walk
    race([&](int t) {
        for (int32_t i = t; i < n; i += kThreads) fal::uf_store<fal::kUfAgent>(&parent[i], fal::uf_find_final<fal::kUfAgent>(parent, i));
    });
    // 3. parent[i] = the smallest node of i's component
    bad += mismatches(name, "roots pass", parent, want);
    if (bad == 0) printf("ok %s: %d nodes, %zu edges\n", name, n, m);
    return bad != 0;
}

}  // namespace

int main() {
    const int32_t n = 3000;
    int failed = 0;
    Edges e;
    for (int32_t i = n - 2; i >= 0; --i) e.push_back({i + 1, i});          // the deep tree that found the halving bug
    failed += run("chain_down", n, e);
    e.clear();
    for (int32_t i = 0; i + 1 < n; ++i) e.push_back({i, i + 1});
    failed += run("chain_up", n, e);
    e.clear();
    for (int32_t i = 1; i < n; ++i) e.push_back({0, i});
    failed += run("star_hub_first", n, e);
    e.clear();
    for (int32_t i = 0; i < n - 1; ++i) e.push_back({n - 1, i});
    failed += run("star_hub_last", n, e);
    e.clear();
    for (int32_t i = 0; i + 2 < n; ++i) e.push_back({i, i + 2});           // odd nodes and even nodes: two components, no more, no fewer
    failed += run("two_chains", n, e);
    e.clear();
    uint64_t x = 0x9E3779B97F4A7C15ull;
    auto next = [&x] { return (int32_t)((x = x * 6364136223846793005ull + 1442695040888963407ull) >> 33) % 4096; };
    for (int k = 0; k < 16384; ++k) {
        const int32_t u = next(), v = next();
        e.push_back({u, v});
    }
    failed += run("random", 4096, e);
    e.clear();
    failed += run("one_node", 1, e);
    e = {{0, 1}, {0, 1}};
    failed += run("two_nodes", 2, e);
    return failed != 0;
}
"""


def plain_compiler():
    """-> argv prefix of a plain host C++ compiler, or None (hipcc compiling the host side does not count: the header takes
    its device form there)"""
    cc = _compiler()
    return None if cc is None or cc[1] else cc[0]


def _compile(tmp_dir, name, source, flags):
    src, exe = os.path.join(str(tmp_dir), name + ".cpp"), os.path.join(str(tmp_dir), name)
    with open(src, "w") as f:
        f.write(source)
    cmd = plain_compiler() + [*flags, "-std=c++17", "-pthread", "-I", CSRC, src, "-o", exe]
    return exe, cmd, subprocess.run(cmd, capture_output=True, text=True)


def sanitizer_missing(tmp_dir):
    """-> why a ThreadSanitizer build cannot be used here (its runtime does not link, or does not start), or None"""
    exe, cmd, r = _compile(tmp_dir, "tsan_probe", "int main() { return 0; }\n", TSAN)
    if r.returncode != 0:
        return "the ThreadSanitizer runtime does not link: " + r.stderr.strip()[-200:]
    r = subprocess.run([exe], capture_output=True, text=True)
    if r.returncode != 0:
        return "a ThreadSanitizer program does not start: " + r.stderr.strip()[-200:]
    return None


def build(tmp_dir, name, flags):
    """compile the program into `tmp_dir`/`name` -> path of the executable"""
    exe, cmd, r = _compile(tmp_dir, name, SOURCE, flags)
    assert r.returncode == 0, f"{' '.join(cmd)}\n{r.stderr[-4000:]}"
    return exe
