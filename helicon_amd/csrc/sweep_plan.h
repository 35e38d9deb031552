// The host arithmetic of the two sweep drivers (sweep_runs / sweep_on_device in helicon_hip.hip, gen_sweep in
// general_host.inc) that needs neither the device nor a context: plain arguments and the standard library only, so
// tests/sweep_plan_check.cpp can run it on its own under the sanitizers.  The two per-size quantities it needs (KT<N>::COLS
// and the fused pass's LDS bytes) come in as an argument and a callable.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <stdexcept>
#include <vector>

constexpr int WALK_RISES = 0, WALK_TWISTS = 1;  // k_fused_pass's candidate loop
constexpr int WALK_PACKED = 2;                  // the pair twist walk with one row transform per pair (N = 512, one segment)

// Whether "auto" (hh_set_fused_walk 0) takes the packed form where its gate holds and choose_walk picks the twist walk
// ("One transform per pair": the measurement that decided it).
constexpr bool AUTO_PACKS_PAIRS = true;

constexpr int64_t HH_MIN_RUN = 8;              // shorter runs do not amortise their table and workgroup granularity
constexpr size_t HH_TABLE_BYTES_MAX = 1ull << 30;

// The fused pass has no intermediate to hold, so its batches are not tied to max_batch: long
// launches even out the tail of the grid (C2: 3.2 M candidates/s at 250 per launch, 3.8 M at 4000).
constexpr int64_t FUSED_BATCH = 131072;       // most candidates per launch (whole runs); 6 GB of column factors + moments at N = 512
constexpr int64_t FUSED_BYTES = 8LL << 30;    // the launch is shortened so that its per-candidate column factors (two halves) fit this

// several segments: candidates per launch of the shared-twist pipelines (q of a batch lives in HBM)
constexpr int64_t SEG_BATCH = 24576;          // most candidates per launch (C5: 11.6 ms at 1024, 9.5 ms at 20k)
constexpr int64_t SEG_BYTES = 12LL << 30;     // ... shortened so that the batch's masked q (0.5 MB per candidate at N = 512) fits this
inline int seg_batch(int n) {
  const int64_t per = (int64_t)(n / 2 + 1) * n * (int64_t)sizeof(float);
  return (int)std::max<int64_t>(1024, std::min<int64_t>(SEG_BATCH, SEG_BYTES / per) / 64 * 64);
}

// The general-size sweep: consecutive runs go into one batch, bounded by GEN_BATCH candidates.
constexpr int64_t GEN_BATCH = 65536;
constexpr int64_t GEN_SEG_BYTES = (int64_t)8 << 30;   // several segments: most bytes of masked q one batch may hold

// words of the ky-major table in the pair layout: two runs to an entry, an odd last run padded to a pair
inline size_t pair_table_words(int64_t runs, int nky, int rows) { return (size_t)((runs + 1) / 2) * 2 * nky * rows; }

// Whether every run of `len` candidates carries run 0's rise column, value for value (at least two runs).  The column
// factors depend on the rise alone (column_factors_of reads neither twist, csym nor rot), so such a list needs one set
// per rise, not one per candidate.  The driver's itertools.product(twists, rises) grid is of this shape.
inline bool rise_columns_shared(const double* hp, int64_t g, int64_t len) {
  if (!hp || len < 1 || g < 2 * len || g % len) return false;
  for (int64_t i = len; i < g; ++i)
    if (!(hp[4 * i + 1] == hp[4 * (i % len) + 1])) return false;
  return true;
}

// Truncation half-window of a ball in pixels: exp(-(rpx apix)^2 / sigma2) < 2^-bits, sigma2 = ball_radius^2 / ln 2
// (hh_set_geometry's value; side: the longer image side).
inline int truncation_rpx(double apix, double ball_radius, int tail_bits, int side) {
  const double sigma2 = ball_radius * ball_radius / std::log(2.0);
  const int bits = tail_bits > 0 ? tail_bits : 24;
  int rpx = (int)std::ceil(std::sqrt(sigma2 * bits * std::log(2.0)) / apix);
  if (rpx < 1) rpx = 1;
  if (rpx > side) rpx = side;
  return rpx;
}

// Whether the simulated lattice is centrosymmetric about the pixel (ny/2, nx/2) for every twist, rise and csym: one unit at
// azimuth 0 and axial offset 0, no tilt, psi or dy.  Lattice point -i of csym copy csym - s is then the mirror of point i of
// copy s, and row ky of the column-transformed image obeys H[ky][nx/2 - a] = conj(H[ky][nx/2 + a]) for |a| < nx/2: a row
// transform that is real up to the term of column 0, whose mirror (column nx) the image does not hold.  Image row 0 has no
// mirror either, so no ball may reach it: radius / apix + rpx + 1 <= ny / 2.  units: n_units x 3 (radius, azimuth,
// axial offset) or NULL for the single unit at (radius, 0, 0).  The candidates' own condition is list_rot_zero.
inline bool geometry_centrosymmetric(int n_units, const double* units, double radius, double dy, bool has_rot, double apix,
                                     int rpx, int ny) {
  if (n_units > 1 || has_rot || !(dy == 0.0) || !(apix > 0.0)) return false;
  double r = radius;
  if (units) {
    if (!(units[1] == 0.0) || !(units[2] == 0.0)) return false;
    r = units[0];
  }
  return std::fabs(r) / apix + (double)rpx + 1.0 <= (double)(ny / 2);
}
// ... and every candidate of the list has rot = 0 (hp: count x 4, the host mirror of the list)
inline bool list_rot_zero(const double* hp, int64_t count) {
  if (!hp || count < 1) return false;
  for (int64_t i = 0; i < count; ++i)
    if (!(hp[4 * i + 3] == 0.0)) return false;
  return true;
}

// Largest |i| a run's table has to cover.  The lattice of utils.py:153 spans ceil(height / rise) indices either side,
// twice what the image holds; a row enters a column's sum only through the window test |x - cx| <= rpx with
// cx = xc inv_apix + N/2 and xc = z_u + i rise, so for x in [0, N - 1] it needs |xc| <= (N/2 + rpx) apix and with it
// |i| rise <= reach = (N/2 + rpx) apix + slack (slack >= |z_u|).  The device evaluates xc and cx in float32: the
// product i rise, the sum with z_u, the product with inv_apix (itself a rounded reciprocal) and the sum with N/2 are
// each off by at most 2^-24 of a magnitude below 2 reach, under 1e-6 reach together.  The bound allows 1e-5 reach and
// one whole index more, so it also holds where reach / rise is an integer or one ulp from it.
inline int64_t table_extent(int nx, double apix, int rpx, double slack, double height, double rise) {
  const double full = std::ceil(height / rise);
  const double reach = ((double)(nx / 2) + (double)rpx) * apix + slack;
  const double cap = std::floor(reach * (1.0 + 1e-5) / rise) + 1.0;
  return (int64_t)std::min(std::min(full, cap), 1048576.0);
}

// How the runs of a launch are cut into workgroups.  The grid is (layers of one run) x ky blocks workgroups, `slots`
// of them resident at a time, each paying a fixed set-up (table slice, weights, twiddles: about four candidates'
// worth) before its candidates; a launch lasts about ceil(workgroups / slots) x (candidates per workgroup + set-up).
// Few, long workgroups amortise the set-up, but the last, partly filled round of a launch costs a whole one.  So the
// runs that fill whole rounds get `groups_a` layers each, and the runs left over for the last round are cut finer
// (`groups_b`), so that round is short.  C2 in one launch (400 runs of 250, 32 ky blocks, 512 slots) is exactly 25
// rounds of whole runs; an eighth of it (50 runs) is 3 rounds of whole runs + 2 runs in 8 pieces each, 798 units
// instead of 4 x 254.
struct FusedSchedule { int runs_a, groups_a, cpw_a, groups_b, cpw_b, layers; double cost; };  // cost: the model's launch length, in candidates
inline FusedSchedule fused_schedule(int64_t runs, int run_len, int n_kb, int slots) {
  const int setup = 4, min_cpw = 16, gmax = std::max(1, run_len / min_cpw);
  auto cpw_of = [&](int g) { return (run_len + g - 1) / g; };
  auto groups_of = [&](int cpw) { return (run_len + cpw - 1) / cpw; };   // even groups: ceil(len / ceil(len / g)) <= g
  FusedSchedule best{};
  double best_t = 1e300;
  for (int ga = 1; ga <= gmax; ++ga) {
    const int cpw_a = cpw_of(ga), ga_e = groups_of(cpw_a);
    const int64_t per_run = (int64_t)ga_e * n_kb;
    const int64_t full = runs * per_run / slots;                          // whole rounds of region A
    const int64_t runs_a = std::min<int64_t>(runs, full * slots / per_run);
    const int64_t runs_b = runs - runs_a;
    const double ta = (double)((runs_a * per_run + slots - 1) / slots) * (cpw_a + setup);
    int gb = ga_e, cpw_b = cpw_a;
    double tb = 0;
    if (runs_b > 0) {
      tb = 1e300;
      for (int g = ga; g <= gmax; ++g) {
        const int cw = cpw_of(g), ge = groups_of(cw);
        const double t = (double)((runs_b * ge * n_kb + slots - 1) / slots) * (cw + setup);
        if (t < tb * 0.995) { tb = t; gb = ge; cpw_b = cw; }
      }
    }
    if (ta + tb < best_t * 0.995) {  // (near-ties go to the fewer, longer workgroups)
      best_t = ta + tb;
      best = FusedSchedule{(int)runs_a, ga_e, cpw_a, gb, cpw_b, (int)(runs_a * ga_e + runs_b * gb), ta + tb};
    }
  }
  return best;
}

// Where the twist walk's workgroups stand in the launch: work id lw = layer x nkb + block in dispatch order -> (ky block
// index kbi, layer gy).  Workgroups are dealt round-robin over the 8 XCDs by id, so ids equal mod 8 (a "class") share an
// L2 and a pool of slots, handed out in id order.  `layers` layers of nkb blocks; the first `la` layers are the long
// workgroups of region A (fused_schedule's runs_a x groups_a), the rest the short pieces of region B.  In id order:
//   [0, la)                    block 0 of every region-A layer;
//   la8 (nkb - 1) more         blocks 1 .. nkb - 1 of the first la8 = la & ~7 layers: each class a contiguous eighth of them
//                              in ky-block-major order, layers ascending inside a block — what an XCD holds at one time is
//                              then consecutive rises of ONE ky block, walking the same table rows at about the same pace;
//   up to la nkb               blocks 1 .. nkb - 1 of the la - la8 layers left over, in dispatch order;
//   [la nkb, la nkb + lb)      block 0 of every region-B layer (lb = layers - la);
//   the rest                   blocks 1 .. nkb - 1 of region B in dispatch order: the short pieces still run last.
// Block 0 leads both regions because its workgroups last longest: their first wavefront owns ky = 0 AND ky = N/2 and
// transforms both, so the workgroup holds its slot for about twice a sibling's time.  Consecutive ids give every class
// its share of them (counts differ by at most one), and first in line they are not what the launch ends on.
// (kbi indexes the launch's list of live ky blocks.  Its entry 0 is always block 0 — hh_set_reference keeps that block
// whatever the mask — so testing kbi == 0 here is testing kb == 0 in the kernel.)
#if defined(__HIPCC__)
#define HH_PLAN_FN __host__ __device__ inline
#else
#define HH_PLAN_FN inline
#endif
struct WalkPlace { int kbi, gy; };
HH_PLAN_FN WalkPlace twist_walk_place(int lw, int nkb, int la, int layers) {
  const int rest = nkb - 1;   // blocks per layer besides block 0
  int first = 0, n = la;      // the region's first layer and its layer count
  const bool region_b = lw >= la * nkb;
  if (region_b) {
    lw -= la * nkb;
    first = la;
    n = layers - la;
  }
  if (lw < n) return WalkPlace{0, first + lw};
  lw -= n;
  const int n8 = region_b ? 0 : n & ~7;   // layers dealt in eighths
  if (lw < n8 * rest) {
    const int j = (lw & 7) * (n8 / 8 * rest) + (lw >> 3);
    return WalkPlace{1 + j / n8, j % n8};
  }
  lw -= n8 * rest;
  return WalkPlace{1 + lw % rest, first + n8 + lw / rest};
}

// The packed pair walk's six sums of a pair (s = 0..2: run A's three moments, s = 3..5: run B's) on their way through the
// wavefront's exchange buffer (tests/packed_reduce_cases.py is this map in numpy).
//   packed_sum_slot        the float lane `lane` stores its sum s to: a row of 64 per sum.
//   packed_sum_first_half  lane L reads floats 8 L .. 8 L + 7 as two 16-byte halves; the half (0: lower, 1: upper) it takes
//                          with its FIRST read.  The LDS serves a 16-byte read in four groups of sixteen lanes, {0-3, 12-15,
//                          20-27}, {4-11, 16-19, 28-31} and the same of lanes 32-63, a group's sixteen reads on the sixteen
//                          4-bank slots of the 64 banks: with lanes 16-31 and 48-63 on the other half every group fills
//                          them once.
//   PACKED_SUM_LANES_A, _B the lanes that store: lane 8 s stores sum s, moment k = s % 3 of candidate ca (A: lanes 0, 8, 16)
//                          or ca + 1 (B: lanes 24, 32, 40) of the workgroup's piece, where that candidate is the piece's.
HH_PLAN_FN int packed_sum_slot(int s, int lane) { return 64 * s + lane; }
HH_PLAN_FN int packed_sum_first_half(int lane) { return (lane >> 4) & 1; }
constexpr unsigned long long PACKED_SUM_LANES_A = 0x010101ull, PACKED_SUM_LANES_B = PACKED_SUM_LANES_A << 24;
#undef HH_PLAN_FN

// Which candidate loop a launch of `runs` whole runs of `run_len` candidates takes when every run shares one rise
// column: the twist walk (workgroups own a rise and walk the runs; fused_schedule with the roles swapped) needs the
// compute unit to hold as many of its workgroups as of the rise walk's (its table rows are double-buffered), and under
// "auto" a schedule whose modelled length is not above the rise walk's — a grid of two or three twists would pay a
// set-up per two or three candidates.  mode: hh_set_fused_walk.  Returns WALK_RISES or WALK_TWISTS.
struct WalkChoice { int walk; FusedSchedule rises, twists; };
inline WalkChoice choose_walk(int64_t runs, int run_len, int n_kb, int slots_rises, int slots_twists, int mode) {
  WalkChoice w{};
  w.walk = WALK_RISES;
  w.rises = fused_schedule(runs, run_len, n_kb, slots_rises);
  if (slots_twists <= 0 || runs < 2 || runs > (int64_t)1 << 30) { w.twists = FusedSchedule{}; return w; }
  w.twists = fused_schedule(run_len, (int)runs, n_kb, slots_twists);
  if (mode == 1 || slots_twists < slots_rises) return w;
  if (mode == 2 || w.twists.cost <= w.rises.cost) w.walk = WALK_TWISTS;
  return w;
}

// What the planning reads of a context and its geometry (apix and slack as the device holds them: float32, widened).
struct SweepGeom {
  int n;             // image side
  double apix;
  int rpx;           // truncation half-window, pixels
  double slack;
  double height;     // nx * apix
  int n_units;
  bool has_rot, table_path, fused_path;
};

// A candidate list the shared-twist first pass can take: runs of `len` consecutive candidates with
// identical (twist, csym, rot) and positive finite rises; run_imax[r] = the subunit index range
// run r's table covers (table_extent of its smallest rise).
struct RunPlan {
  bool ok = false;
  int64_t len = 0;
  int rows = 0;      // table rows per run: (2 max imax + 1) * n_units
  int rows_lds = 0;  // table rows a band of image columns can need (from the smallest rise); 0: too many
  bool fused = false;  // the fused pass fits: whole table slice + column factors in LDS
  int kg = 0;          // fused: table rows per group of four columns
  int rows_f = 0;      // fused: table rows staged per ky
  bool shared_factors = false;  // every run carries run 0's rise column (a twist-major grid): one set of column factors per rise
  std::vector<int> run_imax;
  void reset() {  // as constructed, but run_imax keeps its memory (a plan that is filled sweep after sweep does not allocate)
    std::vector<int> keep = std::move(run_imax);
    keep.clear();
    *this = RunPlan{};
    run_imax = std::move(keep);
  }
};

// The fused pass's shape for a sweep whose smallest rise is rise_all and whose largest table has `rows` rows: table rows
// per group of four columns (subunit indices i with lo <= i rise <= hi, hi - lo = (3 + 2 rpx) apix + 2 slack) and table
// rows staged per ky.  False: the pass does not fit (more than 16 rows per group, or more LDS than a compute unit has).
// fused_lds(rows_f, kg): KF<N>::lds of the context's size.
template <class Lds>
bool fused_shape(const SweepGeom& s, double rise_all, int rows, Lds&& fused_lds, int* kg_out, int* rows_f_out) {
  const double span4 = (3.0 + 2.0 * s.rpx) * s.apix + 2.0 * s.slack;
  const double kg = (std::floor(span4 / (double)(float)rise_all) + 2.0) * s.n_units;
  int rows_f = std::max(rows, (int)std::min(kg, 1.0e6));
  rows_f += (4 - rows_f % 8 + 8) % 8;  // = 4 (mod 8): the eight ky rows of the slice start in different banks
  if (!(kg <= 16.0 && (size_t)fused_lds(rows_f, (int)kg) <= 160 * 1024 - 1024)) return false;
  *kg_out = (int)kg;
  *rows_f_out = rows_f;
  return true;
}

// table_cols: KT<N>::COLS of the context's size.  Fills `plan` in place (plan.ok tells) and returns it.
template <class Lds>
RunPlan& plan_runs(const SweepGeom& s, int table_cols, Lds&& fused_lds, const double* hp, int64_t g, RunPlan& plan) {
  plan.reset();
  if (!hp || !s.table_path || s.has_rot || g < HH_MIN_RUN) return plan;
  int64_t len = 1;
  while (len < g && hp[4 * len] == hp[0] && hp[4 * len + 2] == hp[2] && hp[4 * len + 3] == hp[3]) ++len;
  if (len < HH_MIN_RUN || g % len) return plan;
  const int64_t runs = g / len;
  plan.run_imax.assign((size_t)runs, 0);
  int imax_all = 0;
  double rise_all = INFINITY;
  for (int64_t r = 0; r < runs; ++r) {
    const double* p = hp + 4 * r * len;
    double rise_min = INFINITY;
    for (int64_t k = 0; k < len; ++k) {
      const double* q = p + 4 * k;
      if (!(q[0] == p[0] && q[2] == p[2] && q[3] == p[3])) return plan;
      if (!(q[1] > 0.0) || !(q[1] < INFINITY)) return plan;
      rise_min = std::min(rise_min, q[1]);
    }
    const double im = std::ceil(s.height / rise_min);
    if (im > 1048576.0) return plan;
    const int ext = (int)table_extent(s.n, s.apix, s.rpx, s.slack, s.height, rise_min);
    plan.run_imax[(size_t)r] = ext;
    imax_all = std::max(imax_all, ext);
    rise_all = std::min(rise_all, rise_min);
  }
  // k_first_pass_table: rows = ceil(i1) - floor(i0) + 1 <= (i1 - i0) + 3 with
  // i1 - i0 = ((COLS - 1) apix + 2 rpx apix + 2 slack) / rise; one more row for float32 rounding
  const double span = ((double)(table_cols - 1) + 2.0 * s.rpx) * s.apix + 2.0 * s.slack;
  const double need = (std::floor(span / (double)(float)rise_all) + 4.0) * s.n_units;
  plan.rows_lds = need <= 64.0 ? (int)need : 0;  // KT<N>::ROWS_MAX: one lane per staged row
  plan.rows = (2 * imax_all + 1) * s.n_units;
  if ((size_t)plan.rows * (s.n / 2) * 8 > HH_TABLE_BYTES_MAX) return plan;   // (8: sizeof(float2))
  if (s.fused_path) plan.fused = fused_shape(s, rise_all, plan.rows, fused_lds, &plan.kg, &plan.rows_f);
  if (!plan.fused && plan.rows_lds == 0) return plan;
  plan.shared_factors = plan.fused && rise_columns_shared(hp, g, len);
  if (plan.shared_factors)  // equal columns have equal smallest rises: the shared cgs index ONE table geometry
    for (int64_t r = 1; r < runs; ++r)
      if (plan.run_imax[(size_t)r] != plan.run_imax[0]) throw std::logic_error("plan_runs: equal rise columns with unequal table extents");
  plan.len = len;
  plan.ok = true;
  return plan;
}
template <class Lds>
RunPlan plan_runs(const SweepGeom& s, int table_cols, Lds&& fused_lds, const double* hp, int64_t g) {
  RunPlan plan;
  plan_runs(s, table_cols, fused_lds, hp, g, plan);
  return plan;
}

// A list of n candidates as the sweep takes it: [0, head) and [head + count, n) through the per-candidate transform,
// [head, head + count) — whole runs of plan.len — through the shared-twist pipeline (plan.ok; else count = 0 and head = n).
struct SweepSplit {
  int64_t head = 0, count = 0;
  RunPlan plan;
};

// The whole list where it is whole runs.  Else a list that starts inside a run (a shard cut anywhere) or ends with a
// partial run: the whole runs in the middle still take the shared-twist pipeline, the two ragged ends the general one.
// The run length is that of the first run that starts inside the list; where the runs from there on cannot be planned,
// that of the first run itself (an aligned start, a partial last run).
// Each reading is tried with plan_runs in that order (up to three calls) and the first that can be planned is taken.
// Fills `sp` in place and returns it.
template <class Lds>
SweepSplit& split_sweep(const SweepGeom& s, int table_cols, Lds&& fused_lds, const double* hp, int64_t n, SweepSplit& sp) {
  sp.head = sp.count = 0;
  if (plan_runs(s, table_cols, fused_lds, hp, n, sp.plan).ok) { sp.count = n; return sp; }
  if (hp && s.table_path && !s.has_rot && n >= 2 * HH_MIN_RUN) {
    auto same = [&](int64_t i, int64_t j) {
      return hp[4 * i] == hp[4 * j] && hp[4 * i + 2] == hp[4 * j + 2] && hp[4 * i + 3] == hp[4 * j + 3];
    };
    int64_t head = 1;
    while (head < n && same(head, 0)) ++head;
    int64_t len = 1;
    while (head + len < n && same(head + len, head)) ++len;
    const int64_t count = head < n ? (n - head) / len * len : 0;
    if (head < n && head < len && len >= HH_MIN_RUN && count >= len) {
      if (plan_runs(s, table_cols, fused_lds, hp + 4 * head, count, sp.plan).ok) { sp.head = head; sp.count = count; return sp; }
    }
    // aligned start, partial last run
    len = head;
    const int64_t whole = n / len * len;
    if (len >= HH_MIN_RUN && whole >= len && whole < n) {
      if (plan_runs(s, table_cols, fused_lds, hp, whole, sp.plan).ok) { sp.count = whole; return sp; }
    }
  }
  sp.plan.reset();
  sp.head = n;
  return sp;
}
template <class Lds>
SweepSplit split_sweep(const SweepGeom& s, int table_cols, Lds&& fused_lds, const double* hp, int64_t n) {
  SweepSplit sp;
  split_sweep(s, table_cols, fused_lds, hp, n, sp);
  return sp;
}

// Candidates per launch of sweep_runs, and whether the sweep keeps one set of column factors per rise.
// (never more than the sweep itself holds: the factor and moment buffers are sized by it and only grow)
struct SweepCaps {
  int bmax;
  bool shared;
};
inline SweepCaps sweep_caps(const RunPlan& plan, int max_batch, int n, int n_segments, int64_t count) {
  auto bmax_of = [&](bool shared_sets) {
    // one factor set per rise does not grow with the launch: only FUSED_BATCH and the moments bound it then
    const int fused_cap = shared_sets ? (int)FUSED_BATCH
                                      : (int)std::max<int64_t>(1024, std::min<int64_t>(FUSED_BATCH, FUSED_BYTES / ((int64_t)2 * std::max(1, plan.kg) * n * 4)));
    return !plan.fused ? max_batch
                       : (int)std::min<int64_t>(n_segments == 1 ? std::max(max_batch, fused_cap) : std::max(max_batch, seg_batch(n)),
                                                std::max<int64_t>(count, 16));
  };
  // One set of column factors per rise, computed once for the whole sweep, when every run carries the same rise column
  // and a launch holds whole runs; a run cut into several launches keeps per-launch, per-candidate factors.
  SweepCaps caps{0, plan.fused && plan.shared_factors && count / plan.len >= 2};
  caps.bmax = bmax_of(caps.shared);
  if (caps.shared && plan.len > caps.bmax) {
    caps.shared = false;
    caps.bmax = bmax_of(false);
  }
  return caps;
}

// One launch of sweep_runs: whole runs of one table group, or a piece of one run.
struct SweepBatch {
  int64_t g0;      // first candidate
  int nb;          // candidates
  int64_t r0;      // first run
  int run_len;     // candidates per run inside the batch (a piece of one run counts as one run)
  int64_t q0;      // first run of the table group the batch belongs to
  int nq;          // runs in that group
  bool whole;      // whole runs (false: a piece of a run longer than a launch)
  int half;        // which half of the double-buffered factors and moments it uses: they alternate from 0
};

// The batches of a sweep of `runs` runs of `len` candidates, in order: the tables of as many runs as fit table_bytes
// (and one launch's gridDim.y) form a group, built by one launch ahead of its batches; a group that holds more runs
// than a batch is a whole number of batches.  run_bytes: bytes of one run's table.  The first group is the largest.
inline std::vector<SweepBatch> sweep_batches(int64_t runs, int64_t len, int bmax, size_t run_bytes,
                                             size_t table_bytes = HH_TABLE_BYTES_MAX) {
  const int64_t per_batch = len <= bmax ? bmax / len : 1;
  int64_t per_group = std::max<int64_t>(1, (int64_t)(table_bytes / run_bytes));
  per_group = std::min<int64_t>(std::min<int64_t>(per_group, runs), 65535);
  if (per_group > per_batch) per_group -= per_group % per_batch;
  std::vector<SweepBatch> batches;
  for (int64_t q0 = 0; q0 < runs; q0 += per_group) {
    const int nq = (int)std::min<int64_t>(per_group, runs - q0);
    for (int64_t r0 = q0; r0 < q0 + nq; r0 += per_batch) {
      const int nr = (int)std::min<int64_t>(per_batch, q0 + nq - r0);
      const int64_t first = r0 * len, count = (int64_t)nr * len;
      for (int64_t g0 = first; g0 < first + count; g0 += bmax) {
        const int nb = (int)std::min<int64_t>(bmax, first + count - g0);
        batches.push_back(SweepBatch{g0, nb, r0, (int)std::min<int64_t>(len, nb), q0, nq, len <= bmax, (int)(batches.size() & 1)});
      }
    }
  }
  return batches;
}

// ---- the general-size sweep (gen_sweep) ----------------------------------------------------------------------------------

// several segments in one contraction: the batch is bounded by the bytes of q (kp floats per candidate)
inline int64_t gen_batch_cap(bool seg_contract, size_t kp) {
  return seg_contract ? std::max<int64_t>(64, std::min<int64_t>(GEN_BATCH, GEN_SEG_BYTES / (int64_t)(kp * sizeof(float))) / 64 * 64)
                      : GEN_BATCH;
}

// The runs of one batch: maximal stretches of candidates that share (twist, csym, rot), positions relative to the batch.
struct GenRuns {
  std::vector<int> run_first, run_count, run_imax, run_of;
  int64_t end = 0;            // one past the batch's last candidate in the list
  int imax_all = 0;
  double rise_all = INFINITY;  // the smallest usable rise (INFINITY: none)
};

// The batch that starts at candidate b0 of the n in hp.  A run that would take the batch past batch_cap opens the next
// one; a run longer than a batch is swept in pieces of batch_cap; at most max_runs runs (one launch's gridDim.y).
// False: a rise is too small for the image (more than 2^20 subunit indices either side).
inline bool gen_batch_runs(const double* hp, int64_t n, int64_t b0, int64_t batch_cap, double height, GenRuns& out,
                           int64_t max_runs = 65535) {
  out.run_first.clear(); out.run_count.clear(); out.run_imax.clear(); out.run_of.clear();
  out.rise_all = INFINITY;
  out.imax_all = 0;
  int64_t b1 = b0;
  while (b1 < n && (int64_t)out.run_first.size() < max_runs) {
    const double* p = hp + 4 * b1;
    int64_t len = 1;
    double rise_min = INFINITY;
    auto usable = [](double r) { return r > 0.0 && r < INFINITY; };
    if (usable(p[1])) rise_min = p[1];
    while (b1 + len < n) {
      const double* q = p + 4 * len;
      if (!(q[0] == p[0] && q[2] == p[2] && q[3] == p[3])) break;
      if (usable(q[1])) rise_min = std::min(rise_min, q[1]);
      ++len;
    }
    if (b1 + len - b0 > batch_cap && b1 > b0) break;   // the batch is full: this run opens the next one
    len = std::min<int64_t>(len, batch_cap);            // (a run longer than a batch is swept in pieces)
    const double im = rise_min < INFINITY ? std::ceil(height / rise_min) : 0.0;
    if (im > 1048576.0) return false;
    out.run_first.push_back((int)(b1 - b0));
    out.run_count.push_back((int)len);
    out.run_imax.push_back((int)im);
    for (int64_t k = 0; k < len; ++k) out.run_of.push_back((int)out.run_first.size() - 1);
    out.imax_all = std::max(out.imax_all, (int)im);
    if (rise_min < INFINITY) out.rise_all = std::min(out.rise_all, rise_min);
    b1 += len;
  }
  out.end = b1;
  return true;
}

// Table rows per run, rows per group of four columns and the Stockham row kernel's LDS bytes for a batch's runs
// (nx columns, nxp padded).  ok false: more than 32 table rows per column group.
struct GenSizes {
  bool ok;
  int rows, kg, rows_lds;
  size_t lds;
};
inline GenSizes gen_sizes(const SweepGeom& s, int imax_all, double rise_all, int nx, int nxp) {
  GenSizes z{};
  z.rows = (2 * imax_all + 1) * s.n_units;
  const double span4 = (3.0 + 2.0 * s.rpx) * s.apix + 2.0 * s.slack;
  const double kgd = rise_all < INFINITY ? (std::floor(span4 / (double)(float)rise_all) + 2.0) * s.n_units : 1.0;
  if (kgd > 32.0) return z;
  z.ok = true;
  z.kg = (int)kgd;
  z.rows_lds = std::max(z.rows, z.kg);
  const size_t f2 = 8, f1 = 4;   // sizeof(float2), sizeof(float) and sizeof(int)
  z.lds = (size_t)16 * nxp * f2 + (size_t)8 * z.rows_lds * f2 + (size_t)((nx + 1) & ~1) * f2 + (size_t)z.kg * nxp * f1 +
          (size_t)(nxp / 4 + 4) * f1;
  return z;
}

// The row launch's layers: whole runs while they fill whole rounds of resident workgroups, the runs of the last round
// in shorter pieces (fs: fused_schedule, as for the tuned kernels); one layer per run if the cut-up list would not fit
// the grid (layer_limit).
struct GenLayers {
  std::vector<int> layer_run, layer_first, layer_count;
};
inline void gen_layers(const std::vector<int>& run_first, const std::vector<int>& run_count, const FusedSchedule& fs,
                       GenLayers& out, size_t layer_limit = 65535) {
  const int runs = (int)run_first.size();
  for (int pass = 0; pass < 2; ++pass) {   // (second pass: one layer per run)
    out.layer_run.clear(); out.layer_first.clear(); out.layer_count.clear();
    for (int r = 0; r < runs; ++r) {
      const int groups = pass ? 1 : (r < fs.runs_a ? fs.groups_a : fs.groups_b);
      const int cpw = (run_count[r] + groups - 1) / groups;
      for (int o = 0; o < run_count[r]; o += cpw) {
        out.layer_run.push_back(r);
        out.layer_first.push_back(run_first[r] + o);
        out.layer_count.push_back(std::min(cpw, run_count[r] - o));
      }
    }
    if (out.layer_run.size() <= layer_limit) break;
  }
}
