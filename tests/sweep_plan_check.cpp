// Stand-alone check of helicon_amd/csrc/sweep_plan.h on the host: the cuts and plans of the two sweep drivers against
// brute-force restatements and properties on small random inputs (fixed seed).  Built with -fsanitize=address,undefined
// and run as a child process by tests/test_sweep_plan_host.py.  No GPU, no HIP.
// (fused_schedule and choose_walk are tested through the C ABI: test_host_logic.py, test_twist_walk_host.py.)
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

static std::mt19937 g_rng(20261020u);
static int draw(int lo, int hi) { return std::uniform_int_distribution<int>(lo, hi)(g_rng); }   // inclusive
static double drawf(double lo, double hi) { return std::uniform_real_distribution<double>(lo, hi)(g_rng); }

// ---- the cut of a list into table groups, batches and pieces of a run ---------------------------------------------------
static void check_batches(int64_t runs, int64_t len, int bmax, int per_group_fit) {
  const size_t run_bytes = (size_t)draw(1, 1000) * 8;
  const size_t table_bytes = (size_t)per_group_fit * run_bytes + (size_t)draw(0, (int)run_bytes - 1);
  const std::vector<SweepBatch> b = sweep_batches(runs, len, bmax, run_bytes, table_bytes);
  const int64_t per_batch = len <= bmax ? bmax / len : 1;
  // the largest group the table bytes (and the grid) allow, by search; a whole number of batches where it holds several
  int64_t group = 1;
  for (int64_t k = 1; k <= std::min<int64_t>(runs, 65535); ++k)
    if ((size_t)k * run_bytes <= table_bytes) group = k;
  while (group > per_batch && group % per_batch) --group;
  CHECK(!b.empty());
  int64_t at = 0;
  for (size_t i = 0; i < b.size(); ++i) {
    const SweepBatch& t = b[i];
    CHECK(t.g0 == at);                                  // in order, no gap, no overlap
    CHECK(t.nb >= 1 && t.nb <= bmax);
    CHECK(t.half == (int)(i & 1));
    CHECK(t.q0 % group == 0 && t.nq == (int)std::min<int64_t>(group, runs - t.q0));   // equal groups, a shorter last one
    CHECK(t.q0 <= t.r0 && t.r0 < t.q0 + t.nq);
    CHECK(t.g0 >= t.q0 * len && t.g0 + t.nb <= (t.q0 + t.nq) * len);   // inside its group: a group boundary is a batch boundary
    CHECK(t.whole == (len <= bmax));
    if (t.whole) {   // whole runs of one group
      CHECK(t.g0 == t.r0 * len && t.nb % len == 0 && t.run_len == len && t.run_len == std::min<int64_t>(len, t.nb));
      const int64_t nr = t.nb / len, left = t.q0 + t.nq - t.r0;
      CHECK(nr == std::min(per_batch, left));           // as many as a launch takes, or what is left of the group
      if (t.nq > per_batch && t.q0 + t.nq < runs) CHECK(t.nq % per_batch == 0 && nr == per_batch);
    } else {         // a piece of one run
      CHECK(t.g0 / len == t.r0 && (t.g0 + t.nb - 1) / len == t.r0 && t.run_len == t.nb);
      CHECK(t.nb == bmax || (t.g0 + t.nb) % len == 0);  // full pieces, then what is left of the run
    }
    at += t.nb;
  }
  CHECK(at == runs * len);
  CHECK(b.front().nq == group);                         // the first group is the largest (the drivers size the tables by it)
}

static void check_batches_all() {
  for (int k = 0; k < 3000; ++k) check_batches(draw(1, 40), draw(1, 50), draw(1, 64), draw(1, 7));
  for (int k = 0; k < 200; ++k) {
    const int bmax = draw(1, 49);
    check_batches(draw(1, 40), draw(bmax + 1, 50), bmax, draw(1, 7));   // len > bmax: every run in pieces
    check_batches(draw(1, 40), bmax, bmax, draw(1, 7));                  // len == bmax
    check_batches(1, draw(1, 50), draw(1, 64), draw(1, 7));              // one run
    check_batches(draw(1, 40), draw(1, 50), draw(1, 64), 1);             // one run per group
  }
  const std::vector<SweepBatch> big = sweep_batches(3, 8, 64, (size_t)3 << 30);   // a run's table above the limit: groups of one
  CHECK(big.size() == 3 && big[0].nq == 1 && big[2].q0 == 2);
}

// ---- launch caps ----------------------------------------------------------------------------------------------------------
static void check_caps() {
  const int sizes[6] = {32, 64, 128, 256, 512, 1024};
  for (int k = 0; k < 20000; ++k) {
    RunPlan plan;
    plan.ok = true;
    plan.len = draw(8, 50);
    if (draw(0, 9) == 0) plan.len = draw(1000, 200000);
    plan.fused = draw(0, 3) != 0;
    plan.kg = plan.fused ? draw(1, 16) : 0;
    plan.shared_factors = plan.fused && draw(0, 1);
    const int n = sizes[draw(0, 5)], max_batch = 1 << draw(4, 14), n_segments = draw(1, 3);
    const int64_t runs = draw(0, 3) ? draw(1, 40) : draw(1, 30000), count = runs * plan.len;
    const SweepCaps c = sweep_caps(plan, max_batch, n, n_segments, count);
    if (!plan.fused) {
      CHECK(c.bmax == max_batch && !c.shared);
      continue;
    }
    // restated: the launch holds max_batch or the path's cap, whichever is more, but no more than the sweep (or 16);
    // the cap is seg_batch with several segments, else FUSED_BATCH, cut to the candidates whose two halves of
    // per-candidate factors (2 kg n floats each) fit FUSED_BYTES, but not below 1024
    auto bmax_of = [&](bool shared_sets) {
      int64_t cap = FUSED_BATCH;
      if (n_segments > 1) cap = seg_batch(n);
      else if (!shared_sets) cap = std::max<int64_t>(1024, std::min<int64_t>(FUSED_BATCH, FUSED_BYTES / ((int64_t)2 * plan.kg * n * 4)));
      return std::min<int64_t>(std::max<int64_t>(max_batch, cap), std::max<int64_t>(count, 16));
    };
    const bool want_shared = plan.shared_factors && runs >= 2, fits_shared = plan.len <= bmax_of(true);
    CHECK(c.shared == (want_shared && fits_shared));
    CHECK(c.bmax == bmax_of(c.shared));
    CHECK(c.bmax >= 1 && c.bmax <= std::max<int64_t>(count, 16));
    CHECK(c.bmax <= std::max<int64_t>(max_batch, n_segments == 1 ? FUSED_BATCH : seg_batch(n)));
    if (c.shared) CHECK(runs >= 2 && plan.shared_factors && plan.len <= c.bmax);
    if (!c.shared && n_segments == 1)   // two halves of per-candidate factors fit, but for the floor of 1024 and max_batch
      CHECK((int64_t)2 * c.bmax * plan.kg * n * 4 <= FUSED_BYTES || c.bmax <= std::max(1024, max_batch));
    if (n_segments > 1) CHECK(c.bmax <= std::max(max_batch, seg_batch(n)));
    // shared is given up only where a run does not fit the launch it would get
    RunPlan alone = plan;
    alone.shared_factors = false;
    const SweepCaps u = sweep_caps(alone, max_batch, n, n_segments, count);
    CHECK(!u.shared);
    if (!c.shared) CHECK(c.bmax == u.bmax);
    if (plan.shared_factors && runs >= 2 && !c.shared) CHECK(plan.len > u.bmax);
  }
  RunPlan wide;   // the bytes of the factors are what cuts the launch: N = 1024, 16 rows per group
  wide.ok = wide.fused = true;
  wide.len = 250;
  wide.kg = 16;
  CHECK(sweep_caps(wide, 256, 1024, 1, 100000).bmax == (int)(FUSED_BYTES / (2 * 16 * 1024 * 4)) && FUSED_BYTES / (2 * 16 * 1024 * 4) == 65536);
  CHECK(sweep_caps(wide, 256, 512, 1, 1000000).bmax == FUSED_BATCH);
  CHECK(sweep_caps(wide, 256, 512, 2, 1000000).bmax == seg_batch(512) && seg_batch(512) == 24448 && seg_batch(1024) == 6080);
}

// ---- lists of runs ---------------------------------------------------------------------------------------------------------
struct List {
  std::vector<double> p;   // [n][4]: twist, rise, csym, rot
  int64_t n() const { return (int64_t)p.size() / 4; }
  void add(double twist, double rise, double csym = 1.0, double rot = 0.0) { p.insert(p.end(), {twist, rise, csym, rot}); }
  bool same(int64_t i, int64_t j) const { return p[4 * i] == p[4 * j] && p[4 * i + 2] == p[4 * j + 2] && p[4 * i + 3] == p[4 * j + 3]; }
};
// a key that differs from the run before in one of twist, csym, rot
static void next_key(double key[3]) { key[draw(0, 2)] += 1.0; }

static const SweepGeom GEOM{64, 1.0, 1, 1e-3, 64.0, 1, false, true, false};   // every rise >= 2 can be planned (8 table columns)
static const int COLS = 8;
static size_t small_lds(int, int) { return 1000; }
static size_t no_lds(int, int) { return (size_t)1 << 20; }

static void check_ragged() {
  for (int k = 0; k < 4000; ++k) {
    const int L = draw(1, 50), R = draw(1, 40);
    const int cut_head = draw(0, 2) ? draw(0, L - 1) : 0, cut_tail = draw(0, 2) ? draw(0, L - 1) : 0;
    List full;
    double key[3] = {10.0, 1.0, 0.0};
    for (int r = 0; r < R; ++r, next_key(key))
      for (int i = 0; i < L; ++i) full.add(key[0], drawf(2.0, 10.0), key[1], key[2]);
    if ((int64_t)cut_head + cut_tail >= full.n()) continue;
    List list;
    list.p.assign(full.p.begin() + 4 * cut_head, full.p.end() - 4 * cut_tail);
    const int64_t n = list.n();
    const SweepSplit sp = split_sweep(GEOM, COLS, no_lds, list.p.data(), n);
    static SweepSplit reused;   // the in-place form the driver uses, filled list after list: the same answer
    split_sweep(GEOM, COLS, no_lds, list.p.data(), n, reused);
    CHECK(reused.head == sp.head && reused.count == sp.count && reused.plan.ok == sp.plan.ok && reused.plan.len == sp.plan.len &&
          reused.plan.rows == sp.plan.rows && reused.plan.rows_lds == sp.plan.rows_lds && reused.plan.run_imax == sp.plan.run_imax);
    int stretches = 1;
    for (int64_t i = 1; i < n; ++i) stretches += !list.same(i, i - 1);
    // three ranges that partition the list
    CHECK(sp.head >= 0 && sp.count >= 0 && sp.head + sp.count <= n);
    // The driver's first reading is kept: a list that is whole runs of its first stretch's length is taken whole — also
    // where that stretch is a cut-off head that divides the runs behind it (8 + 16 + 16: five runs of 8).
    const RunPlan plain = plan_runs(GEOM, COLS, no_lds, list.p.data(), n);
    if (L >= HH_MIN_RUN && !cut_head && !cut_tail) CHECK(plain.ok && plain.len == L);   // an aligned list: empty ends
    if (plain.ok) {
      CHECK(sp.plan.ok && sp.head == 0 && sp.count == n && sp.plan.len == plain.len && sp.plan.run_imax == plain.run_imax);
      if (stretches == 1) CHECK(plain.len == n);
      continue;
    }
    if (stretches == 1) CHECK(n < HH_MIN_RUN);
    if (!sp.plan.ok) {
      CHECK(sp.count == 0 && sp.head == n);
    } else {   // the middle: whole runs of one length, each of one (twist, csym, rot), each starting at a change
      const int64_t len = sp.plan.len;
      CHECK(len >= HH_MIN_RUN && sp.count >= len && sp.count % len == 0 && (int64_t)sp.plan.run_imax.size() == sp.count / len);
      for (int64_t i = sp.head; i < sp.head + sp.count; ++i) {
        const int64_t first = sp.head + (i - sp.head) / len * len;
        CHECK(list.same(i, first));
        if (i == first && i > 0) CHECK(!list.same(i, i - 1));
      }
      if (sp.head > 0) CHECK(sp.head < len);                          // a cut-off run, not whole runs left out
      CHECK(n - sp.head - sp.count < len);
    }
    const int head_piece = cut_head ? L - cut_head : 0;                // what the cuts left of the first and the last run
    const int64_t whole = (n - head_piece) / L;
    if (L < HH_MIN_RUN || n < 2 * HH_MIN_RUN) CHECK(!sp.plan.ok);   // short runs, or a short ragged list: no middle
    if (L >= HH_MIN_RUN && whole >= 1 && n >= 2 * HH_MIN_RUN)
      CHECK(sp.plan.ok && sp.plan.len == L && sp.head == head_piece && sp.count == whole * L);
  }
  List rot;
  for (int i = 0; i < 32; ++i) rot.add(i / 16, 3.0);
  SweepGeom g = GEOM;
  CHECK(split_sweep(g, COLS, no_lds, rot.p.data(), 32).count == 32);
  g.has_rot = true;
  CHECK(split_sweep(g, COLS, no_lds, rot.p.data(), 32).head == 32);
  g = GEOM;
  g.table_path = false;
  CHECK(split_sweep(g, COLS, no_lds, rot.p.data(), 32).head == 32);
  CHECK(split_sweep(GEOM, COLS, no_lds, nullptr, 32).head == 32);    // a device-only list
}

static void check_plan_runs() {
  for (int k = 0; k < 3000; ++k) {
    SweepGeom g = GEOM;
    g.n_units = draw(1, 3);
    g.fused_path = draw(0, 1);
    const int L = draw(8, 50), R = draw(1, 40);
    const bool shared = draw(0, 2) == 0;
    List list;
    std::vector<double> rise_min((size_t)R, INFINITY), column;
    for (int i = 0; i < L; ++i) column.push_back(drawf(2.0, 10.0));
    double key[3] = {10.0, 1.0, 0.0};
    for (int r = 0; r < R; ++r) {
      if (draw(0, 3)) next_key(key);                                   // (equal neighbours are two runs all the same)
      for (int i = 0; i < L; ++i) {
        const double rise = shared ? column[(size_t)i] : drawf(2.0, 10.0);
        list.add(key[0], rise, key[1], key[2]);
        rise_min[(size_t)r] = std::min(rise_min[(size_t)r], rise);
      }
    }
    int64_t len = 1;   // what the first run's length reads as
    while (len < list.n() && list.same(len, 0)) ++len;
    const RunPlan plan = plan_runs(g, COLS, small_lds, list.p.data(), list.n());
    if (len != L) {    // equal keys in front: another run length, or none that divides the list into runs of one key
      if (plan.ok) CHECK(plan.len == len && list.n() % len == 0);
    } else {
      CHECK(plan.ok && plan.len == L && (int)plan.run_imax.size() == R);
      int imax = 0;
      for (int r = 0; r < R && plan.ok; ++r) {
        CHECK(plan.run_imax[(size_t)r] == (int)table_extent(g.n, g.apix, g.rpx, g.slack, g.height, rise_min[(size_t)r]));
        imax = std::max(imax, plan.run_imax[(size_t)r]);
      }
      CHECK(plan.rows == (2 * imax + 1) * g.n_units);
      CHECK(plan.fused == g.fused_path);                               // kg <= (floor(5.002 / 2) + 2) * 3 = 12
      CHECK(plan.shared_factors == (plan.fused && shared && R >= 2));
      if (plan.shared_factors)
        for (int r = 1; r < R; ++r) CHECK(plan.run_imax[(size_t)r] == plan.run_imax[0]);
      if (plan.fused) CHECK(plan.rows_f >= plan.rows && plan.rows_f % 8 == 4 && plan.kg >= 2 * g.n_units && plan.kg <= 16);
      // what spoils it: one bad rise, one candidate of another key, in-plane rotation, a partial run at the end
      const int64_t at = draw(0, (int)list.n() - 1);
      const double bad[4] = {0.0, -1.0, INFINITY, NAN};
      List l2 = list;
      l2.p[(size_t)(4 * at + 1)] = bad[draw(0, 3)];
      CHECK(!plan_runs(g, COLS, small_lds, l2.p.data(), l2.n()).ok);
      if (at % L) {    // inside a run (a change at a run's first candidate is a legitimate list)
        l2 = list;
        l2.p[(size_t)(4 * at + (draw(0, 1) ? 0 : 2))] += 0.5;
        CHECK(!plan_runs(g, COLS, small_lds, l2.p.data(), l2.n()).ok);
      }
      SweepGeom g2 = g;
      g2.has_rot = true;
      CHECK(!plan_runs(g2, COLS, small_lds, list.p.data(), list.n()).ok);
      CHECK(!plan_runs(g, COLS, small_lds, list.p.data(), list.n() - draw(1, L - 1)).ok || R == 1);   // g % len != 0
      if (R == 1) CHECK(plan_runs(g, COLS, small_lds, list.p.data(), list.n() - 1).ok == (L - 1 >= HH_MIN_RUN));
    }
  }
  // neither first pass fits: no fused shape (LDS) and more table rows than a band's lanes
  List fine;
  for (int i = 0; i < 16; ++i) fine.add(1.0, 0.1 + 0.01 * i);
  SweepGeom g = GEOM;
  g.fused_path = true;
  CHECK(!plan_runs(g, COLS, no_lds, fine.p.data(), 16).ok);
  // a table above HH_TABLE_BYTES_MAX
  g = SweepGeom{1024, 1.0, 10, 1e-3, 1024.0, 1, false, true, true};
  List tiny;
  for (int i = 0; i < 16; ++i) tiny.add(1.0, 0.001);
  CHECK(!plan_runs(g, 16, small_lds, tiny.p.data(), 16).ok);
  CHECK(!plan_runs(GEOM, COLS, small_lds, fine.p.data(), 7).ok);       // shorter than HH_MIN_RUN
}

// ---- the general-size sweep: the runs of a batch, the layers of its row launch --------------------------------------------
static void check_gen() {
  for (int k = 0; k < 3000; ++k) {
    const int R = draw(1, 40), cap = draw(1, 64), max_runs = draw(0, 2) ? 65535 : draw(1, 7);
    const double height = 200.0;
    List list;
    double key[3] = {10.0, 1.0, 0.0};
    for (int r = 0; r < R; ++r) {
      if (draw(0, 4)) next_key(key);                                   // (equal neighbours merge into one run)
      for (int i = 0, L = draw(1, 50); i < L; ++i) list.add(key[0], draw(0, 9) ? drawf(1.0, 20.0) : (draw(0, 1) ? -1.0 : INFINITY), key[1], key[2]);
    }
    const int64_t n = list.n();
    GenRuns gr;
    GenLayers gl;
    for (int64_t b0 = 0; b0 < n;) {
      CHECK(gen_batch_runs(list.p.data(), n, b0, cap, height, gr, max_runs));
      const int64_t nb = gr.end - b0;
      const int runs = (int)gr.run_first.size();
      CHECK(nb >= 1 && runs >= 1 && runs <= max_runs && (nb <= cap || runs == 1));
      CHECK((int)gr.run_count.size() == runs && (int)gr.run_imax.size() == runs && (int64_t)gr.run_of.size() == nb);
      int at = 0, imax_all = 0;
      double rise_all = INFINITY;
      for (int r = 0; r < runs; ++r) {   // the runs tile the batch; run_of is their inverse
        CHECK(gr.run_first[(size_t)r] == at && gr.run_count[(size_t)r] >= 1 && gr.run_count[(size_t)r] <= cap);
        double rise_min = INFINITY;
        for (int i = at; i < at + gr.run_count[(size_t)r]; ++i) {
          CHECK(gr.run_of[(size_t)i] == r && list.same(b0 + i, b0 + at));
          const double rise = list.p[(size_t)(4 * (b0 + i) + 1)];
          if (rise > 0.0 && rise < INFINITY) rise_min = std::min(rise_min, rise);
        }
        at += gr.run_count[(size_t)r];
        // a run ends at the list's end, at a change, or at the cap (a run longer than a batch is cut there)
        CHECK(b0 + at == n || !list.same(b0 + at, b0 + at - 1) || gr.run_count[(size_t)r] == cap);
        // (a run cut at the cap sees the rises of the whole stretch: its table covers at least its own)
        const int im = gr.run_imax[(size_t)r];
        CHECK(im >= (rise_min < INFINITY ? (int)std::ceil(height / rise_min) : 0));
        if (b0 + at == n || !list.same(b0 + at, b0 + at - 1)) CHECK(im == (rise_min < INFINITY ? (int)std::ceil(height / rise_min) : 0));
        imax_all = std::max(imax_all, im);
        if (rise_min < INFINITY) rise_all = std::min(rise_all, rise_min);
      }
      CHECK(at == nb && gr.imax_all == imax_all && gr.rise_all <= rise_all);
      if (gr.end < n && runs < max_runs) {   // the batch is full: the next run would pass the cap
        int64_t next = 1;
        while (gr.end + next < n && list.same(gr.end + next, gr.end)) ++next;
        CHECK(nb + next > cap);
      }
      // layers: whatever the schedule, the layers of a run tile it, in order
      FusedSchedule fs{};
      fs.runs_a = draw(0, runs);
      fs.groups_a = draw(1, 5);
      fs.groups_b = draw(1, 5);
      for (int low = 0; low < 2; ++low) {
        size_t cut_up = 0;
        for (int r = 0; r < runs; ++r) {
          const int groups = r < fs.runs_a ? fs.groups_a : fs.groups_b, cpw = (gr.run_count[(size_t)r] + groups - 1) / groups;
          cut_up += (size_t)((gr.run_count[(size_t)r] + cpw - 1) / cpw);
        }
        const size_t limit = low ? (size_t)runs : 65535;
        gen_layers(gr.run_first, gr.run_count, fs, gl, limit);
        const size_t layers = gl.layer_run.size();
        CHECK(gl.layer_first.size() == layers && gl.layer_count.size() == layers);
        CHECK(layers == (cut_up <= limit ? cut_up : (size_t)runs));     // a low limit: exactly one layer per run
        size_t l = 0;
        for (int r = 0; r < runs; ++r) {
          int o = 0;
          for (; l < layers && gl.layer_run[l] == r; ++l) {
            CHECK(gl.layer_first[l] == gr.run_first[(size_t)r] + o && gl.layer_count[l] >= 1);
            o += gl.layer_count[l];
          }
          CHECK(o == gr.run_count[(size_t)r]);
        }
        CHECK(l == layers);
      }
      b0 = gr.end;
    }
  }
  List small;   // more than 2^20 subunit indices either side
  for (int i = 0; i < 4; ++i) small.add(1.0, i == 2 ? 1e-5 : 5.0);
  GenRuns gr;
  CHECK(!gen_batch_runs(small.p.data(), 4, 0, 64, 200.0, gr));
  CHECK(gen_batch_cap(false, 0) == GEN_BATCH && gen_batch_cap(true, 512) == GEN_BATCH);
  CHECK(gen_batch_cap(true, (size_t)1 << 20) == 2048 && gen_batch_cap(true, (size_t)1 << 30) == 64);
  // sizes: 120 x 200 at apix 2, rpx 2, slack 1e-3, smallest rise 3: span4 = 14.002, kg = 6; the LDS sum by hand
  const SweepGeom g{0, 2.0, 2, 1e-3, 400.0, 1, false, true, true};
  const GenSizes z = gen_sizes(g, 40, 3.0, 200, 208);
  CHECK(z.ok && z.rows == 81 && z.kg == 6 && z.rows_lds == 81);
  CHECK(z.lds == (size_t)16 * 208 * 8 + 8 * 81 * 8 + 200 * 8 + 6 * 208 * 4 + (208 / 4 + 4) * 4);
  const GenSizes z1 = gen_sizes(g, 0, INFINITY, 200, 208);               // no usable rise: one row per group
  CHECK(z1.ok && z1.rows == 1 && z1.kg == 1 && z1.rows_lds == 1);
  CHECK(!gen_sizes(g, 40, 0.45, 200, 208).ok && gen_sizes(g, 40, 0.47, 200, 208).kg == 31);   // more than 32 rows per group
}

// ---- the lists of tests/test_gpu_sweep_run_cuts.py cross the cuts they are meant to -----------------------------------------
static void check_gpu_test_lists() {
  // side 256 at 1 A, half-window 1 px, 3,000 runs of the rises 0.360 ... 0.374: three table groups
  const SweepGeom g{256, 1.0, 1, 1e-3, 256.0, 1, false, true, true};
  List list;
  for (int r = 0; r < 3000; ++r)
    for (int i = 0; i < 8; ++i) list.add(20.0 + 0.01 * r, 0.36 + 0.002 * i);
  const RunPlan plan = plan_runs(g, 16, small_lds, list.p.data(), list.n());
  CHECK(plan.ok && plan.fused && plan.shared_factors && plan.len == 8 && plan.rows == 719 && plan.kg == 15 && plan.rows_f == 724);
  const SweepCaps caps = sweep_caps(plan, 256, 256, 1, list.n());
  CHECK(caps.shared && caps.bmax == 24000);
  const size_t run_bytes = (size_t)plan.rows * 128 * 8;
  CHECK(run_bytes == 736256);
  const std::vector<SweepBatch> b = sweep_batches(3000, 8, caps.bmax, run_bytes);
  CHECK(b.size() == 3 && b[0].nq == 1458 && b[1].q0 == 1458 && b[1].nq == 1458 && b[2].q0 == 2916 && b[2].nq == 84);
  CHECK(b[0].nb == 1458 * 8 && b[2].g0 == 2916 * 8 && b[2].nb == 84 * 8 && b[0].whole);
  // side 32 at 2 A, two segments, one run of 60,000 rises: three launches, per-launch factors in alternating halves
  const SweepGeom g32{32, 2.0, 10, 1e-3, 64.0, 1, false, true, true};
  List one;
  for (int i = 0; i < 60000; ++i) one.add(28.0, 6.0 + 8.0 * i / 59999.0);
  const RunPlan p1 = plan_runs(g32, 16, small_lds, one.p.data(), one.n());
  CHECK(p1.ok && p1.fused && !p1.shared_factors && p1.len == 60000);
  const SweepCaps c1 = sweep_caps(p1, 256, 32, 2, one.n());
  CHECK(!c1.shared && c1.bmax == 24576);
  const std::vector<SweepBatch> b1 = sweep_batches(1, p1.len, c1.bmax, (size_t)p1.rows * 16 * 8);
  CHECK(b1.size() == 3 && b1[0].nb == 24576 && b1[1].nb == 24576 && b1[2].nb == 10848 && !b1[0].whole);
  CHECK(b1[0].half == 0 && b1[1].half == 1 && b1[2].half == 0 && b1[2].r0 == 0 && b1[2].run_len == 10848);
}

int main() {
  check_gpu_test_lists();
  check_batches_all();
  check_caps();
  check_ragged();
  check_plan_runs();
  check_gen();
  if (g_failed) {
    std::printf("sweep_plan_check: %d checks failed\n", g_failed);
    return 1;
  }
  std::printf("sweep_plan_check: ok\n");
  return 0;
}
