// What a persistent recurrence launch will be, decided on the host in plain C++ (no HIP header, no device code): which
// kernel instantiation a shape gets, how its grid is laid over the XCDs, how much of an XCD it holds, and whether it may
// run beside the persistent grids in flight.  ft_rnn_persist.hip puts the HIP calls around these functions;
// tests/test_rnn_plan_cpu.py and tests/cpp/rnn_plan_main.cpp hold them to their reference without a GPU.
#pragma once
#include <stddef.h>
#include <stdlib.h>

#include <vector>

namespace rnn_plan {

// as the kernels have them (ft_rnn_persist.hip asserts the equality)
constexpr int NSH = 16, CSTRIDE = 32, NFLAG = 256, NXCC = 64, MB16 = 16, GCH = 8;
inline int cdiv(long a, long b) { return (int)((a + b - 1) / b); }

// The FT_RNN_* switches of ONE launch: each is looked up the first time the plan asks for it, so a launch reads a
// switch at most once and only where it decides something.  env = getenv in the library, any table in a test.
struct Switches {
  enum Id { B3, FWD_UB16, FWD_NW4, GRU_WIDE, MB, BWD_RS, XCDMAP, SIG, XCDALIGN, LOCAL, GRANULES, GRAN4, FAST_CELL, DEBUG,
            ADMIT_PCT, COUNT };
  const char* (*env)(const char*);
  int val[COUNT];
  bool known[COUNT] = {};
  explicit Switches(const char* (*e)(const char*)) : env(e) {}
  int operator[](Id i) {
    static const struct { const char* name; int dflt; } def[COUNT] = {
        {"FT_RNN_B3", 1}, {"FT_RNN_FWD_UB16", 1}, {"FT_RNN_FWD_NW4", 1}, {"FT_RNN_GRU_WIDE", 1}, {"FT_RNN_MB", 8},
        {"FT_RNN_BWD_RS", 1}, {"FT_RNN_XCDMAP", 1}, {"FT_RNN_SIG", 1}, {"FT_RNN_XCDALIGN", 1}, {"FT_RNN_LOCAL", 1},
        {"FT_RNN_GRANULES", 1}, {"FT_RNN_GRAN4", 1}, {"FT_RNN_FAST_CELL", 1}, {"FT_RNN_DEBUG", 0},
        {"FT_RNN_ADMIT_PCT", 100}};
    if (!known[i]) {
      const char* e = env ? env(def[i].name) : nullptr;
      val[i] = e ? atoi(e) : def[i].dflt;
      known[i] = true;
    }
    return val[i];
  }
};

// workspace = [arrival counters | flag words | XCC ids | exchange buffer (fp32 parities, granule parities)]; the sync
// region (and, for the all-gather forms, the exchange buffer) is zeroed per call from the allocation's start (the fault
// word is NOT in here: it is the device-global g_rnn_fault, which launches never touch)
struct Carve { size_t sync_bytes, xb_bytes, total_bytes; };      // the exchange buffer starts at sync_bytes
inline size_t sync_region_bytes(int ngrp) { return (size_t)ngrp * (NSH * CSTRIDE + NFLAG + NXCC) * sizeof(unsigned); }
inline Carve carve(int ngrp, size_t xb) { return {sync_region_bytes(ngrp), xb, sync_region_bytes(ngrp) + xb}; }
// two fp32 parities, then the granule area of the XCD-local split kernels (two parities of 8-byte granules)
inline Carve carve_ws(int ngrp, int K, int mb) {
  return carve(ngrp, (size_t)3 * 2 * ngrp * (K / 4) * mb * 4 * sizeof(float));
}
// reduce-scatter backward: xb[parity][group][consumer][producer][16 * mb]
inline Carve carve_ws_rs(int ngrp, int nchunks, int mb) {
  return carve(ngrp, (size_t)2 * ngrp * nchunks * nchunks * 16 * mb * sizeof(float));
}
// ft_rnn_workspace: the largest of every form's workspace, in 16 and 8 rows per workgroup (8 rows: as many or fewer
// padded rows, but up to twice the groups' sync words)
inline size_t workspace_bound(int gates, int B, int H) {
  size_t m = 0;
  for (int mb : {MB16, 8}) {
    const int ngrp = 2 * cdiv(B, mb);
    for (size_t b : {carve_ws(ngrp, H, mb).total_bytes, carve_ws(ngrp, gates * H, mb).total_bytes,
                     carve_ws_rs(ngrp, H / 16, mb).total_bytes})
      m = b > m ? b : m;
  }
  return m;
}

// Batch rows per workgroup of the forms that come in an 8-row variant (the 512-wide LSTM's forward and reduce-scatter
// BPTT, the 256-wide GRU's forward and all-gather BPTT), for nd * ceil(B / 16) (direction, batch group) groups.  Every
// group runs on one XCD slot of its own, so with fewer than 8 groups the 16-row form leaves slots idle (B = 32: 4 of 8);
// 8 rows give the same batch twice the groups, each CU half the rows to load, multiply and update per step, with the
// same results bit for bit.  Only where the 8-row groups still fit one per slot and are more of them.  The narrower
// GRUs (the predictors, H <= 128) stay on 16 rows: not measured.  FT_RNN_MB=16 (read per launch): always 16 rows.
inline int rows_per_wg(int nd, int B, Switches& sw) {
  if (sw[Switches::MB] == 16) return 16;
  const int g16 = nd * cdiv(B, 16), g8 = nd * cdiv(B, 8);
  return g16 < 8 && g8 <= 8 && g8 > g16 ? 8 : 16;
}

// The form of a launch.  v: the kernel's template arguments as the FT_RNN_DEBUG line prints them -- FWD <G, NW, B3, UB,
// BC, MB>, BWD (all-gather) <G, NW, GW, B3, MB>, BWD_RS (reduce-scatter) <G, NW, NT, MB>, the unused slots -1; gran: the
// kernel has the granule form of the XCD-local hand-off (the others hand over through flag words there).  PER_STEP: the
// persistent form does not apply and the caller issues the per-step kernels.
enum Kind { PER_STEP, FWD, BWD, BWD_RS };
struct Form {
  Kind kind;
  int v[6];
  int threads, rows, nchunks, nbg, total;      // chunks per group, batch groups, workgroups that have work
  int gran, xcd_aware, sig_per_wave;
  Carve ws;
  size_t zero_bytes;                           // of the workspace's start, before the launch
};
inline const char* kind_name(Kind k) { return k == FWD ? "fwd" : k == BWD ? "bwd" : k == BWD_RS ? "bwd_rs" : "per-step"; }

inline Form finish(Form f, Kind kind, int nd, int B, size_t ws_bytes, Switches& sw) {
  f.threads = f.v[1] * 64;
  f.nbg = cdiv(B, f.rows);
  f.total = nd * f.nbg * f.nchunks;            // nd = 1: the forward direction's groups only (the workspace keeps two)
  f.xcd_aware = sw[Switches::XCDMAP];
  f.sig_per_wave = sw[Switches::SIG];
  // only the sync region (counters, flags, XCC ids) of the reduce-scatter form needs zeroing: every exchange block is
  // written before it is read
  f.zero_bytes = kind == BWD_RS ? f.ws.sync_bytes : f.ws.total_bytes;
  f.kind = ws_bytes < f.ws.total_bytes || f.ws.xb_bytes >= (1ull << 31) ? PER_STEP : kind;
  return f;
}

inline Form plan_fwd(int G, int H, int B, int ND, int T, bool vec, size_t ws_bytes, Switches& sw) {
  Form f = {};
  if (T < 2 || !vec || H % 16 != 0) return f;
  const int ngroups = H / 16;
  int NW = ngroups > 16 ? 8 : 4;
  // The 512-wide LSTM: a (direction, batch group) group must fit ONE XCD to hand over through its L2, i.e. at most 32
  // workgroup-CUs.  Two forms do: (a) 16 units per 8-wave workgroup (32 workgroups, one per CU; 2 resident k-blocks per
  // wave, granule hand-off) -- every CU then pulls the group's h once per step instead of twice (two 8-unit workgroups
  // per CU: 64 KB per CU and step through one 64 B/clk path) -- and (b) 8 units per 4-wave workgroup (64 workgroups, two
  // per CU; 4 resident blocks per wave, flag words).  Round 2 measured (a) at 5.65 us per step against 3.77: it spilled
  // 57 registers.  With ONE MFMA site per (block, tile) for all hand-off protocols (round 3) it spills 4 and runs 3.51
  // against 3.88 in isolation, 22.8 -> 22.3 ms per train step (profiles/r03_rnn_ab.txt).  FT_RNN_FWD_UB16=0: form (b).
  const bool wide = NW == 8 && G == 4 && H / 8 > 32 && H % 32 == 0 && cdiv(H / 32, 8) <= 2 && sw[Switches::B3] &&
                    sw[Switches::FWD_UB16];
  if (!wide && NW == 8 && G == 4 && H % 32 == 0 && cdiv(H / 32, 4) <= 4 && sw[Switches::FWD_NW4]) NW = 4;
  if (cdiv(ngroups, NW) > GCH) return f;
  const int bpw = H % 32 == 0 ? cdiv(H / 32, NW) : 99;                    // 32-k blocks per wave in the split form
  // matmul on the bf16 pipe (exact split): the 8-wave kernels keep at most 2 resident k-blocks per wave (BC), the 4-wave
  // ones 4 -- a width beyond that (8 waves: H = 544 .. 1024) takes the f32 form, whose 8 k-groups per wave cover it
  const bool b3 = bpw <= (NW == 8 ? 2 : 4) && sw[Switches::B3];
  // GRU, H = 256 (the trunk's two GRUs; the postnet's runs 841 steps): 8 waves with ONE resident k-block each and 16
  // hidden units per workgroup -- 16 producers per group instead of 32, half the operand bytes per wave.  Same box,
  // us per step at T = 841 (lab/gru256_ab.py): 4 waves x 2 blocks x 8 units 2.03 | 8 x 1 x 8: 2.03-2.07 | 4 x 2 x 16:
  // 2.04 | 8 x 1 x 16: 1.78-1.81 | 8 x 1 x 32: 2.30.  FT_RNN_GRU_WIDE=0: the 4-wave 8-unit form.
  const bool gru_wide = G == 3 && H == 256 && b3 && NW == 4 && sw[Switches::GRU_WIDE];
  const bool ub16 = wide || gru_wide;
  f.rows = ub16 ? rows_per_wg(ND, B, sw) : MB16;
  const int BC = wide ? 2 : (gru_wide || !b3 || bpw <= 1) ? 1 : bpw <= 2 ? 2 : 4;
  const int v[6] = {G, ub16 ? 8 : NW, ub16 || b3, ub16 ? 16 : 8, BC, f.rows};
  for (int i = 0; i < 6; ++i) f.v[i] = v[i];
  f.gran = v[2] && BC <= 2;
  f.nchunks = H / v[3];
  f.ws = carve_ws(2 * cdiv(B, f.rows), H, f.rows);
  return finish(f, FWD, ND, B, ws_bytes, sw);
}

// BPTT, both directions.  rs: try the reduce-scatter form (H/16 output tiles over NW waves, NT tiles each) before the
// all-gather one; the caller plans again without it when the reduce-scatter grid is refused admission.
inline Form plan_bwd(int G, int H, int B, int T, bool vec, size_t ws_bytes, Switches& sw, bool rs = true) {
  Form f = {};
  if (T < 2 || !vec || H % 16 != 0) return f;
  const int K = G * H, ngroups = K / 16, tiles = H / 16;
  // waves x resident K groups per wave: 8 waves keep up to 16 groups each (256 registers per lane at 2 waves per
  // SIMD); 16 waves would cap a lane at 128 registers and spill the LSTM-512 working set
  const int NW = ngroups > 128 ? 16 : (ngroups > 16 ? 8 : 4);
  const int GW = ngroups > 64 ? 16 : 8;
  if (cdiv(ngroups, NW) > GW) return f;
  f.nchunks = tiles;
  // measured (lab/rnn_step_us.py, B = 32, us/step, all-gather -> reduce-scatter): LSTM H=512 5.26 -> 4.67;
  // GRU H=256 3.15 -> 3.60, H=128 2.87 -> 2.95, H=64 2.70 -> 2.73: the form pays once the gathered operand is large
  // (G*H >= 1024 values per row); FT_RNN_BWD_RS=2 forces it wherever it applies
  const bool rs_tiles = tiles == 4 || tiles == 8 || tiles == 16 || tiles == 32;
  if (rs && rs_tiles && sw[Switches::BWD_RS] && sw[Switches::B3] && sw[Switches::SIG]) {
    // the LSTM-512 form (G = 4, 32 tiles) comes in 8 rows per workgroup too (rows_per_wg), which regroups the batch
    f.rows = G == 4 && tiles == 32 ? rows_per_wg(2, B, sw) : MB16;
    f.ws = carve_ws_rs(2 * cdiv(B, f.rows), tiles, f.rows);
    const int v[6] = {G, tiles == 4 ? 4 : 8, tiles <= 8 ? 1 : tiles / 8, f.rows, -1, -1};
    for (int i = 0; i < 6; ++i) f.v[i] = v[i];
    const Form r = finish(f, BWD_RS, 2, B, ws_bytes, sw);
    if (r.kind == BWD_RS && (sw[Switches::BWD_RS] == 2 || K >= 1024)) return r;
  }
  // (GRU H = 256, K = 768 on 16 waves with 2 of the 24 k-blocks each instead of 8 x 3: 11.9 us per step against 2.45 --
  //  a 1024-thread workgroup caps a lane at 128 registers; 12 waves x 2 blocks: 5.1 us; lab/gru256_ab.py)
  const bool b3 = K % 32 == 0 && cdiv(K / 32, NW) <= GW / 2 && sw[Switches::B3];
  // the GRU-256 form (8 waves x 3 resident k-blocks) comes in 8 rows per workgroup too (rows_per_wg): regroup the batch
  f.rows = G == 3 && H == 256 && b3 && NW == 8 && GW == 8 ? rows_per_wg(2, B, sw) : MB16;
  f.ws = carve_ws(2 * cdiv(B, f.rows), K, f.rows);
  const int v[6] = {G, NW, GW, b3, f.rows, -1};
  for (int i = 0; i < 6; ++i) f.v[i] = v[i];
  f.gran = b3 && GW / 2 <= 4;
  return finish(f, BWD, 2, B, ws_bytes, sw);
}

// Grid layout of a persistent launch.  The 1-D grid is 8 x per: the decode hands XCD slot x the work items
// [x*per, (x+1)*per).  ALIGNED: per = whole (direction, batch group) groups, so that a group's hand-off stays inside
// one XCD (the XCD-local protocol then applies; surplus workgroups of the larger grid exit at once); successive
// launches start on different slots (rotor: the caller's count of groups placed so far).  SPREAD: per = ceil(total / 8),
// groups straddle XCDs, agent-scope protocol only.  The aligned layout is tried first; the spread one only runs when the
// aligned per-XCD demand exceeds a whole XCD (admission makes a launch WAIT for conflicting ones rather than refuse it,
// so a demand <= 1 is always taken as aligned).  grid 0: the layout does not apply.
struct Layout { int grid, per, xcd_off, aligned; };
inline int aligned_per(const Form& f) { return f.nchunks * cdiv(f.total / f.nchunks, 8); }
inline Layout layout_aligned(const Form& f, Switches& sw, int& rotor) {
  if (!f.xcd_aware || !f.sig_per_wave || !sw[Switches::XCDALIGN] || f.nchunks > NXCC) return {0, 0, 0, 0};
  const int ngroups = f.total / f.nchunks, off = rotor & 7;
  rotor += ngroups < 8 ? ngroups : 8;
  return {8 * aligned_per(f), aligned_per(f), off, 1};
}
inline Layout layout_spread(const Form& f) { return {8 * cdiv(f.total, 8), cdiv(f.total, 8), 0, 0}; }

// share of one XCD's CUs a launch holds: (workgroups of the fullest XCD slot) / (CUs of an XCD x workgroups per CU,
// capped at 2 to stay well inside what the dispatcher really admits); -1: the occupancy is not known
inline double demand(int wgs_per_slot, int per_cu, int cus) {
  if (per_cu < 1) return -1.0;
  return (double)wgs_per_slot / ((per_cu > 2 ? 2 : per_cu) * (cus / 8.0));
}

// Admission (the why: ft_rnn_persist.hip).  fl: the unfinished launches, each with .stream, .d (its demand) and
// .joined_by (streams that waited for .stream after it was enqueued).  A launch of demand d on `stream` is REFUSED if it
// does not fit the chip even alone (d > 1 x scale; the per-step kernels run); it is admitted while
//     d + sum over the OTHER streams of (the largest d among that stream's unfinished launches) <= 0.75 x scale
// or nothing of another stream is unfinished; otherwise it is admitted AFTER `stream` has waited for the launches
// listed in wait_for (indices into fl: exactly those that counted).  scale = FT_RNN_ADMIT_PCT / 100.
enum Verdict { REFUSE, ADMIT, ADMIT_AFTER_WAIT };
struct Admission {
  Verdict verdict;
  std::vector<size_t> wait_for;
};
template <typename FlightT, typename StreamT>
Admission admission(const std::vector<FlightT>& fl, StreamT stream, double d, double scale) {
  if (d < 0.0 || d > 1.0 || d > 1.0 * scale) return {REFUSE, {}};
  auto counts = [&](const FlightT& f) {
    if (f.stream == stream) return false;
    for (const auto& j : f.joined_by)
      if (j == stream) return false;
    return true;
  };
  double others = 0.0;
  for (size_t i = 0; i < fl.size(); ++i) {
    if (!counts(fl[i])) continue;
    bool first = true;
    double mx = 0.0;
    for (size_t j = 0; j < fl.size(); ++j)
      if (fl[j].stream == fl[i].stream && counts(fl[j])) {
        if (j < i) first = false;
        if (fl[j].d > mx) mx = fl[j].d;
      }
    if (first) others += mx;
  }
  if (others == 0.0 || d + others <= 0.75 * scale) return {ADMIT, {}};
  Admission a = {ADMIT_AFTER_WAIT, {}};
  for (size_t i = 0; i < fl.size(); ++i)
    if (counts(fl[i])) a.wait_for.push_back(i);
  return a;
}

}  // namespace rnn_plan
