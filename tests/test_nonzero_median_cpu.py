"""The median selection shared by the input-conditioning kernels (nonzero_median<N> in badslam_amd/csrc/preprocess_kernels.hpp),
compiled for the host as it stands in the header and compared with a sort-based statement of the rule (sort the non-zero
values; odd count: the middle one; even count: the lower middle one if it is strictly nearer to the fp32 mean, else the
upper one) on random windows of 4, 9, 16 and 64 values: uniform, clustered just below 65535, clustered at small values,
clustered so that ties and near-ties are frequent, with every fill ratio from empty to full."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HARNESS_HEAD = r"""
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>
#define __device__
#define __forceinline__ inline
using std::min;
"""

HARNESS_TAIL = r"""
static uint32_t by_sorting(const std::vector<uint32_t>& all, uint32_t* count) {
  std::vector<uint16_t> v;
  for (uint32_t x : all) if (x) v.push_back((uint16_t)x);
  *count = (uint32_t)v.size();
  if (v.empty()) return 0;
  std::sort(v.begin(), v.end());
  if (v.size() % 2) return v[v.size() / 2];
  float sum = 0;
  for (uint16_t x : v) sum += x;
  const float average = sum / v.size();
  const float low_diff = std::fabs(v[v.size() / 2 - 1] - average), high_diff = std::fabs(v[v.size() / 2] - average);
  return low_diff < high_diff ? v[v.size() / 2 - 1] : v[v.size() / 2];
}
template <int N> long run(std::mt19937& rng, int trials) {
  long bad = 0;
  for (int t = 0; t < trials; ++t) {
    uint32_t v[N];
    std::vector<uint32_t> all(N);
    const int mode = rng() % 5;
    const uint32_t base = mode == 1 ? 65535 - rng() % 8 : (mode == 2 ? 1 + rng() % 8 : 10 + rng() % 65000);
    for (int i = 0; i < N; ++i) {
      uint32_t x;
      if (mode == 0) x = rng() % 65536;
      else if (mode == 3) x = base + rng() % 3;
      else if (mode == 4) x = base + (rng() % 2) * (rng() % 400);
      else x = std::min<uint32_t>(65535, std::max<int>(1, (int)base + (int)(rng() % 4) - (mode == 1 ? 3 : 0)));
      if (rng() % 100 < (unsigned)(t % 101)) x = 0;
      v[i] = all[i] = std::min<uint32_t>(x, 65535);
    }
    uint32_t count_a, count_b;
    const uint32_t want = by_sorting(all, &count_b), got = nonzero_median<N>(v, &count_a);
    if (count_a != count_b || (count_b && want != got)) {
      if (bad < 5) std::printf("N=%d: sorting gives %u, selection gives %u (counts %u / %u)\n", N, want, got, count_b, count_a);
      ++bad;
    }
  }
  return bad;
}
int main() {
  std::mt19937 rng(1);
  const long bad = run<4>(rng, 400000) + run<9>(rng, 400000) + run<16>(rng, 200000) + run<64>(rng, 60000);
  std::printf("mismatches: %ld\n", bad);
  return bad != 0;
}
"""


def selection_source():
    text = open(os.path.join(ROOT, "badslam_amd", "csrc", "preprocess_kernels.hpp")).read()
    start = text.index("template <int N>\n__device__ __forceinline__ uint32_t nonzero_median")
    end = text.index("\n}\n", start) + 3
    return text[start:end]


def test_selection_agrees_with_sorting(tmp_path):
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to compile the selection for the host")
    source = tmp_path / "harness.cpp"
    source.write_text(HARNESS_HEAD + selection_source() + HARNESS_TAIL)
    binary = tmp_path / "harness"
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", str(source), "-o", str(binary)], check=True)
    done = subprocess.run([str(binary)], capture_output=True, text=True)
    assert done.returncode == 0 and "mismatches: 0" in done.stdout, done.stdout + done.stderr
