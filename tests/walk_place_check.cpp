// Stand-alone check of twist_walk_place (helicon_amd/csrc/sweep_plan.h) on the host: where the twist walk's workgroups
// stand in a launch.  The map must be a bijection onto (ky block index, layer), lead each region with block 0 in
// consecutive ids (so the eight residue classes mod 8 — the XCDs — share the slow workgroups evenly), keep the contiguous
// eighths of the other blocks, and leave region B behind region A.  Built with -fsanitize=address,undefined and run as a
// child process by tests/test_walk_place_host.py.  No GPU, no HIP.
#include "sweep_plan.h"

#include <cstdio>
#include <random>

static int g_failed = 0;
#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      if (g_failed < 20) std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      ++g_failed;                                                          \
    }                                                                      \
  } while (0)

static std::mt19937 g_rng(20261021u);
static int draw(int lo, int hi) { return std::uniform_int_distribution<int>(lo, hi)(g_rng); }   // inclusive

// The map this one replaces (k_fused_pass's remap until now): the first la8 layers in eighths over ALL blocks, the rest
// in dispatch order.
static WalkPlace old_place(int lw, int nkb, int la) {
  const int la8 = la & ~7;
  if (lw < la8 * nkb) {
    const int j = (lw & 7) * (la8 / 8 * nkb) + (lw >> 3);
    return WalkPlace{j / la8, j % la8};
  }
  return WalkPlace{lw % nkb, lw / nkb};
}

// la: layers of region A (runs_a x groups_a), lb: layers of region B
static void check_shape(int nkb, int la, int lb) {
  const int layers = la + lb, total = layers * nkb, rest = nkb - 1, la8 = la & ~7, m = la8 * rest;
  std::vector<int> seen((size_t)total, 0);
  int a0[8] = {}, b0[8] = {};            // block-0 workgroups of region A and B per residue class
  std::vector<int> next_j(8, -1);        // per class: the next place in ky-block-major order of blocks 1 .. nkb - 1
  std::vector<int> eighth_used(8, 0);
  for (int lw = 0; lw < total; ++lw) {
    const WalkPlace p = twist_walk_place(lw, nkb, la, layers);
    CHECK(p.kbi >= 0 && p.kbi < nkb && p.gy >= 0 && p.gy < layers);
    if (!(p.kbi >= 0 && p.kbi < nkb && p.gy >= 0 && p.gy < layers)) return;
    ++seen[(size_t)p.gy * nkb + p.kbi];
    const bool in_a = lw < la * nkb;
    CHECK(in_a == (p.gy < la));                       // region B's short pieces still run last
    const int cls = lw & 7;
    if (in_a) {
      CHECK((p.kbi == 0) == (lw < la));               // block 0 has the region's lowest ids
      if (p.kbi == 0) {
        ++a0[cls];
        CHECK(p.gy == lw);
      } else if (lw < la + m) {                       // each class: a contiguous eighth, ky-block-major, layers ascending
        const int j = (p.kbi - 1) * la8 + p.gy;
        CHECK(p.gy < la8);
        if (next_j[(size_t)cls] < 0) {
          CHECK(j % (m / 8) == 0);
          CHECK(!eighth_used[(size_t)(j / (m / 8))]);
          eighth_used[(size_t)(j / (m / 8))] = 1;
        } else {
          CHECK(j == next_j[(size_t)cls]);
        }
        next_j[(size_t)cls] = j + 1;
      } else {                                        // the layers that do not fill eighths: dispatch order
        const int r = lw - la - m;
        CHECK(p.gy == la8 + r / rest && p.kbi == 1 + r % rest);
      }
    } else {
      const int r = lw - la * nkb;
      CHECK((p.kbi == 0) == (r < lb));
      if (p.kbi == 0) {
        ++b0[cls];
        CHECK(p.gy == la + r);
      } else {
        CHECK(p.gy == la + (r - lb) / rest && p.kbi == 1 + (r - lb) % rest);
      }
    }
  }
  for (int v : seen) CHECK(v == 1);                   // a bijection onto what the dispatch-order grid covers
  int a_lo = a0[0], a_hi = a0[0], a_sum = 0, b_sum = 0;
  for (int c = 0; c < 8; ++c) {
    a_lo = std::min(a_lo, a0[c]);
    a_hi = std::max(a_hi, a0[c]);
    a_sum += a0[c];
    b_sum += b0[c];
    CHECK(b0[c] <= (lb + 7) / 8);
    if (m > 0) CHECK(next_j[(size_t)c] >= 0 && next_j[(size_t)c] % (m / 8) == 0);   // each class walked a whole eighth
  }
  CHECK(a_sum == la && b_sum == lb);
  CHECK(a_hi - a_lo <= 1);
}

// C2: 400 runs of 250 rises, 32 ky blocks, 512 slots; the twist walk schedules rises as "runs" of 400
static void check_c2() {
  const int nkb = 32;
  const FusedSchedule fs = fused_schedule(250, 400, nkb, 512);
  CHECK(fs.runs_a == 240 && fs.groups_a == 1 && fs.groups_b == 8 && fs.cpw_b == 50 && fs.layers == 320);
  const int la = fs.runs_a * fs.groups_a, lb = fs.layers - la;
  check_shape(nkb, la, lb);
  // the defect, pinned: the old map puts every block-0 workgroup of both regions into ONE residue class
  int old_a[8] = {}, old_b[8] = {};
  for (int lw = 0; lw < fs.layers * nkb; ++lw) {
    const WalkPlace p = old_place(lw, nkb, la);
    if (p.kbi == 0) ++(p.gy < la ? old_a : old_b)[lw & 7];
  }
  CHECK(old_a[0] == 240 && old_b[0] == 80);
  for (int c = 1; c < 8; ++c) CHECK(old_a[c] == 0 && old_b[c] == 0);
  // the other blocks: a class still walks whole ky blocks one after the other.  31 blocks of 240 over 8 classes are 930
  // places = 3.875 blocks each, so a class holds at least 3 whole blocks, touches at most 5, and no block is cut more
  // than once.
  std::vector<std::vector<int>> per_block(8, std::vector<int>((size_t)nkb, 0));
  for (int lw = la; lw < la * nkb; ++lw) {
    const WalkPlace p = twist_walk_place(lw, nkb, la, fs.layers);
    ++per_block[(size_t)(lw & 7)][(size_t)p.kbi];
  }
  std::vector<int> owners((size_t)nkb, 0);
  for (int c = 0; c < 8; ++c) {
    int whole = 0, touched = 0, lo = nkb, hi = -1;
    for (int k = 1; k < nkb; ++k) {
      const int v = per_block[(size_t)c][(size_t)k];
      if (v > 0) { ++touched; ++owners[(size_t)k]; lo = std::min(lo, k); hi = std::max(hi, k); }
      if (v == la) ++whole;
    }
    CHECK(per_block[(size_t)c][0] == 0);
    CHECK(whole >= 3 && touched <= 5 && touched == hi - lo + 1);   // consecutive blocks, whole but for the two ends
    for (int k = lo + 1; k < hi; ++k) CHECK(per_block[(size_t)c][(size_t)k] == la);
  }
  for (int k = 1; k < nkb; ++k) CHECK(owners[(size_t)k] >= 1 && owners[(size_t)k] <= 2);
}

// an eighth of C2: 50 runs of 250 rises
static void check_c2_eighth() {
  const int nkb = 32;
  const FusedSchedule fs = fused_schedule(250, 50, nkb, 512);
  CHECK(fs.layers >= 1 && fs.runs_a * fs.groups_a <= fs.layers);
  check_shape(nkb, fs.runs_a * fs.groups_a, fs.layers - fs.runs_a * fs.groups_a);
}

int main() {
  check_c2();
  check_c2_eighth();
  for (int i = 0; i < 4000; ++i) {
    const int nkb = draw(1, 33);
    int la = draw(0, 60) * draw(1, 8);               // (no region A: a launch below one round of slots)
    int lb = draw(0, 9) * draw(1, 8);
    if (la + lb == 0) la = draw(1, 60);
    check_shape(nkb, la, lb);
  }
  for (int nkb = 1; nkb <= 33; ++nkb)                 // every block count at the sizes where a remainder appears
    for (int la = 0; la <= 17; ++la) check_shape(nkb, la, la % 3);
  if (g_failed) {
    std::printf("walk_place_check: %d check(s) failed\n", g_failed);
    return 1;
  }
  std::printf("walk_place_check: ok\n");
  return 0;
}
