// Stand-alone host test of csrc/ft_rnn_plan.h (tests/test_rnn_plan_cpu.py builds it with the sanitizers and runs it):
// the admission decision on hand-built flight lists, the aligned layout's rotor and the workspace carve.
#include <stdio.h>
#include <string.h>

#include "ft_rnn_plan.h"

using namespace rnn_plan;

static int g_failed = 0;
#define CHECK(cond)                                             \
  do {                                                          \
    if (!(cond)) {                                              \
      fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
      ++g_failed;                                               \
    }                                                           \
  } while (0)

struct Flight {
  int stream;
  double d;
  std::vector<int> joined_by;
};
using Flights = std::vector<Flight>;
using Wait = std::vector<size_t>;

static void test_admission() {
  const int me = 1;
  // nothing in flight: up to a whole XCD
  CHECK(admission(Flights{}, me, 1.0, 1.0).verdict == ADMIT);
  CHECK(admission(Flights{}, me, 0.01, 1.0).verdict == ADMIT);
  CHECK(admission(Flights{}, me, 1.03125, 1.0).verdict == REFUSE);
  CHECK(admission(Flights{}, me, -1.0, 1.0).verdict == REFUSE);                  // occupancy unknown
  // launches of the same stream run in order: they do not count, however many
  CHECK(admission(Flights{{me, 1.0, {}}, {me, 1.0, {}}}, me, 1.0, 1.0).verdict == ADMIT);
  // neither does a launch this stream has already waited for
  CHECK(admission(Flights{{2, 1.0, {me}}}, me, 1.0, 1.0).verdict == ADMIT);
  CHECK(admission(Flights{{2, 1.0, {3}}}, me, 0.5, 1.0).verdict == ADMIT_AFTER_WAIT);  // (joined by another stream only)
  // several unfinished launches of ONE other stream count once, at their largest demand
  const Flights one = {{2, 0.25, {}}, {2, 0.5, {}}, {2, 0.125, {}}};
  CHECK(admission(one, me, 0.25, 1.0).verdict == ADMIT);                         // 0.25 + 0.5, not + 0.875
  CHECK(admission(one, me, 0.5, 1.0).verdict == ADMIT_AFTER_WAIT);
  // two other streams add up
  const Flights two = {{2, 0.25, {}}, {3, 0.25, {}}};
  CHECK(admission(two, me, 0.25, 1.0).verdict == ADMIT);                         // 0.75: the edge of the budget
  CHECK(admission(two, me, 0.375, 1.0).verdict == ADMIT_AFTER_WAIT);
  // the 0.75 budget at its edge
  CHECK(admission(Flights{{2, 0.5, {}}}, me, 0.25, 1.0).verdict == ADMIT);
  CHECK(admission(Flights{{2, 0.25, {}}}, me, 0.5, 1.0).verdict == ADMIT);
  CHECK(admission(Flights{{2, 0.5, {}}}, me, 0.5, 1.0).verdict == ADMIT_AFTER_WAIT);
  CHECK(admission(Flights{{2, 0.5, {}}}, me, 0.25, 1.0).wait_for.empty());
  // the wait list names exactly the flights that counted: not this stream's, not the joined one, every other -- the
  // smaller launches of a stream too (the stream then follows all of them)
  const Flights mix = {{me, 1.0, {}}, {2, 0.5, {}}, {3, 0.5, {me}}, {2, 0.125, {}}, {4, 0.25, {3}}};
  const Admission a = admission(mix, me, 0.5, 1.0);
  CHECK(a.verdict == ADMIT_AFTER_WAIT && a.wait_for == (Wait{1, 3, 4}));
  CHECK(admission(mix, 3, 0.5, 1.0).wait_for == (Wait{0, 1, 3}));                // stream 4 was joined by 3
  // a stream's launches that no longer count do not lend it their demand: 0.5 of stream 2 is joined, 0.125 is not
  CHECK(admission(Flights{{2, 0.5, {me}}, {2, 0.125, {}}}, me, 0.625, 1.0).verdict == ADMIT);
  // FT_RNN_ADMIT_PCT scales both bounds; beyond the scaled whole XCD a launch is refused, never made to wait
  CHECK(admission(Flights{}, me, 0.04, 0.04).verdict == ADMIT);
  CHECK(admission(Flights{}, me, 0.05, 0.04).verdict == REFUSE);
  CHECK(admission(Flights{{2, 0.5, {}}}, me, 0.05, 0.04).verdict == REFUSE);
  CHECK(admission(Flights{}, me, 0.5, 0.5).verdict == ADMIT);
  CHECK(admission(Flights{{2, 0.25, {}}}, me, 0.5625, 0.5).verdict == REFUSE);
  CHECK(admission(Flights{{2, 0.125, {}}}, me, 0.25, 0.5).verdict == ADMIT);       // 0.375 = 0.75 x 0.5
  CHECK(admission(Flights{{2, 0.25, {}}}, me, 0.25, 0.5).verdict == ADMIT_AFTER_WAIT);
  CHECK(admission(Flights{{2, 0.5, {}}}, me, 0.5, 2.0).verdict == ADMIT);          // 1.0 <= 1.5
  CHECK(admission(Flights{{2, 1.0, {}}}, me, 1.0, 2.0).verdict == ADMIT_AFTER_WAIT);
  CHECK(admission(Flights{}, me, 1.5, 2.0).verdict == REFUSE);                   // a grid must still fit one XCD's CUs
}

static const char* no_env(const char*) { return nullptr; }
static const char* no_align(const char* name) { return strcmp(name, "FT_RNN_XCDALIGN") ? nullptr : "0"; }

static Form form_of(int nchunks, int groups) {
  Form f = {};
  f.kind = BWD;
  f.nchunks = nchunks;
  f.total = groups * nchunks;
  f.xcd_aware = f.sig_per_wave = 1;
  return f;
}

static void test_layouts() {
  Switches sw(no_env);
  // four groups per launch (the decoder LSTM at B = 32 in 16 rows): slots 0-3, then 4-7, and again
  int rotor = 0;
  for (int want : {0, 4, 0, 4, 0}) {
    const Layout l = layout_aligned(form_of(32, 4), sw, rotor);
    CHECK(l.aligned == 1 && l.xcd_off == want && l.per == 32 && l.grid == 256);
  }
  // eight groups (or more) take every slot: the start does not move
  rotor = 0;
  for (int groups : {8, 8, 12, 8}) CHECK(layout_aligned(form_of(16, groups), sw, rotor).xcd_off == 0);
  CHECK(rotor == 32);
  CHECK(layout_aligned(form_of(16, 12), sw, rotor).per == 32);                   // two rounds of slots
  // mixed: 3, 4, 8 and 2 groups
  rotor = 0;
  const int groups[] = {3, 4, 8, 2, 3}, off[] = {0, 3, 7, 7, 1};
  for (int i = 0; i < 5; ++i) CHECK(layout_aligned(form_of(8, groups[i]), sw, rotor).xcd_off == off[i]);
  // where the aligned layout does not apply the rotor stays
  const int before = rotor;
  CHECK(layout_aligned(form_of(65, 2), sw, rotor).grid == 0);                    // more chunks than published XCC ids
  Form f = form_of(8, 2);
  f.sig_per_wave = 0;
  CHECK(layout_aligned(f, sw, rotor).grid == 0);
  f = form_of(8, 2);
  f.xcd_aware = 0;
  CHECK(layout_aligned(f, sw, rotor).grid == 0);
  Switches off_sw(no_align);
  CHECK(layout_aligned(form_of(8, 2), off_sw, rotor).grid == 0 && rotor == before);
  const Layout s = layout_spread(form_of(34, 6));                                // 204 workgroups
  CHECK(s.per == 26 && s.grid == 208 && s.xcd_off == 0 && s.aligned == 0);
  // demand: workgroups of a slot over the 32 CUs of an XCD x workgroups per CU, at most 2 of them
  CHECK(demand(32, 1, 256) == 1.0 && demand(32, 2, 256) == 0.5 && demand(32, 5, 256) == 0.5 && demand(16, 1, 256) == 0.5);
  CHECK(demand(33, 1, 256) > 1.0 && demand(8, 0, 256) == -1.0 && demand(8, 1, 128) == 0.5);
}

static void test_carve() {
  // sync region of a group: 16 counter shards a 128-B line apart, 256 flag words, 64 XCC ids
  CHECK(sync_region_bytes(1) == (16 * 32 + 256 + 64) * 4 && sync_region_bytes(4) == 13312);
  const Carve f = carve_ws(4, 512, 16);          // LSTM-512 forward, B = 32 in 16 rows: 3 x 2 x [4][128][16][4] floats
  CHECK(f.sync_bytes == 13312 && f.xb_bytes == 786432 && f.total_bytes == 13312 + 786432);
  const Carve r = carve_ws_rs(8, 32, 8);         // its reduce-scatter BPTT in 8 rows: 2 x [8][32][32][16 * 8] floats
  CHECK(r.sync_bytes == 26624 && r.xb_bytes == 8388608 && r.total_bytes == 26624 + 8388608);
  CHECK(workspace_bound(4, 32, 512) == 26624 + 8388608);      // (larger than both all-gather carves)
  // the plan carves with the same functions and zeroes what the form needs zeroed
  Switches sw(no_env);
  const Form fw = plan_fwd(4, 512, 32, 2, 100, true, (size_t)-1, sw);
  CHECK(fw.kind == FWD && fw.rows == 8 && fw.ws.total_bytes == carve_ws(8, 512, 8).total_bytes && fw.zero_bytes == fw.ws.total_bytes);
  const Form bw = plan_bwd(4, 512, 32, 100, true, (size_t)-1, sw);
  CHECK(bw.kind == BWD_RS && bw.ws.total_bytes == r.total_bytes && bw.zero_bytes == r.sync_bytes);
  CHECK(plan_bwd(4, 512, 32, 100, true, r.total_bytes - 1, sw).kind == BWD);     // too small for it: the all-gather form
  CHECK(plan_fwd(4, 512, 32, 2, 100, true, fw.ws.total_bytes - 1, sw).kind == PER_STEP);
  CHECK(plan_fwd(4, 512, 32, 2, 1, true, (size_t)-1, sw).kind == PER_STEP);
  CHECK(plan_fwd(4, 512, 32, 2, 100, false, (size_t)-1, sw).kind == PER_STEP);
  CHECK(plan_fwd(3, 16 * 8 * 8 + 16, 4, 2, 100, true, (size_t)-1, sw).kind == PER_STEP);      // more than GCH groups per wave
}

int main() {
  test_admission();
  test_layouts();
  test_carve();
  if (g_failed) fprintf(stderr, "%d checks failed\n", g_failed);
  return g_failed ? 1 : 0;
}
