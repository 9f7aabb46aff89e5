// bfs(pp, s) and pagerank(pp, v) on a PPPCSR (host/bfs.h, host/pagerank.h -> pppcsr_bfs / pppcsr_pagerank on the device)
// against the generic host templates bfs<PPPCSR> / pagerank<PPPCSR, float>, which walk the partitions through
// get_neighbourhood / getNode one call per vertex.  Levels equal, PageRank equal bit for bit.  Built and run by
// tests/test_gpu_pppcsr_consumers.py (-m gpu).
#include <cstdio>
#include <cstring>
#include <vector>

#include "PPPCSR.h"
#include "bfs.h"
#include "pagerank.h"

static int failures = 0;
#define EXPECT_TRUE(c) do { if (!(c)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); failures++; } } while (0)

static void check(PPPCSR &pp, const std::vector<uint32_t> &starts, const char *label) {
  const uint64_t n = pp.get_n();
  for (uint32_t s : starts) {
    const std::vector<uint32_t> dev = bfs(pp, s), host = bfs<PPPCSR>(pp, s);
    EXPECT_TRUE(dev.size() == n && dev == host);
    if (dev != host) std::printf("  %s: bfs from %u differs\n", label, s);
  }
  std::vector<float> w(n);
  for (uint64_t v = 0; v < n; v++) w[v] = 0.25f + (float)(v % 11) / 3.0f;
  for (const std::vector<float> &vals : {w, std::vector<float>(n, 1.0f)}) {
    const std::vector<float> dev = pagerank(pp, vals), host = pagerank<PPPCSR, float>(pp, vals);
    EXPECT_TRUE(dev.size() == n && host.size() == n && std::memcmp(dev.data(), host.data(), n * sizeof(float)) == 0);
  }
}

int main() {
  PCSR::quiet() = true;
  const uint32_t n = 2000;
  PPPCSR pp(n, n, true, 1, 4, false);
  uint64_t x = 12345;
  auto rnd = [&]() {
    x = x * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(x >> 33);
  };
  for (int i = 0; i < 12000; i++) pp.add_edge(rnd() % n, rnd() % n, 1 + (uint32_t)i);
  for (int i = 0; i < 600; i++) pp.add_edge(1500, rnd() % n, 7);  // a vertex of high degree in the last partition
  for (int i = 0; i < 3000; i++) pp.remove_edge(rnd() % n, rnd() % n);  // (mostly missing: num_neighbors drops below the degree)
  check(pp, {0, 777, 1500, n - 1}, "4 partitions");
  pp.add_node();
  pp.add_edge(n, 5, 1);
  pp.add_edge(3, n, 1);
  check(pp, {0, n, 1999}, "after add_node");
  std::printf(failures ? "FAILED (%d)\n" : "ALL PASSED\n", failures);
  return failures ? 1 : 0;
}
