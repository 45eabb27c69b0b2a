// Stand-alone dump of a batch schedule (csrc/dtc_schedule.h) -- the
// autocorrelator's, the energy sweep's or the sampling sweep's -- host only, no
// GPU:
//
//   g++ -std=c++17 -O1 -D__HIP_PLATFORM_AMD__ -I <rocm>/include -I <pkg>/csrc
//       tools/schedule_check.cpp -o schedule_check
//   ./schedule_check [key=value ...]
//
// builds the schedule of one case as the engine's autocorr_impl would (the same
// RunCfg, SchedOpts and SchedReq, five fake buffer addresses) and prints the
// canonical listing: one line per launch (dump_schedule), the builder's
// SchedInfo, the wavefront table-set keys in order, and a tally.  The defaults
// are the headline line (L = 20, T = 30, x kicks, depolarizing noise, the octet
// layout, every option at its default).  Keys:
//   L T t_offset t_first probe n_sub n_pre octet      integers (probe -1: L / 2)
//   kick=x|y|xy_cycle|xy_cycle5|gen     noise=none|depol|device|bond|device_bond
//   zsite energy want_fwd want_echo                   0 / 1
//   lightcone lc_wide lc_wide3 dual runahead wavefront split13   0 / 1;  wf_cap
//   mode=autocorr|energy|sample   energy: build_energy_schedule as energy_impl
//     calls it, sample: build_sample_schedule as dtc_sample does (noise none or
//     depol); the buffers are F, E and vals, and the tally adds the launches
//     that leave a time's state (t_state) and the Z, XPost and XPre parts
// tests/test_schedule_cpu.py compares the dumps with tests/golden/schedules.json
// (it may also be built with -fsanitize=address,undefined and run as it is).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "dtc_schedule.h"

using namespace dtc::sched;

static int usage(const char* what) {
  std::fprintf(stderr, "schedule_check: %s\n", what);
  return 2;
}

// The kick table of a case: row r, site i, sub-gate q as {re, im} x 4.  x: RX
// matrices, y: RY (real) matrices, xy_cycle: rows alternate between the two,
// xy_cycle5: five RX rows, five RY rows, ... (the package's xy_cycle kicks:
// RX for (r / 5) even), gen: sub-gate q alternates (a product outside both
// families).
static std::vector<double> kick_table(const std::string& pat, int n_rows, int L, int n_sub) {
  std::vector<double> k((size_t)n_rows * L * n_sub * 8, 0.0);
  for (int r = 0; r < n_rows; ++r)
    for (int i = 0; i < L; ++i)
      for (int q = 0; q < n_sub; ++q) {
        const bool y = pat == "y" || (pat == "xy_cycle" && (r & 1)) ||
                       (pat == "xy_cycle5" && ((r / 5) & 1)) || (pat == "gen" && (q & 1)) ||
                       (pat == "gen" && n_sub == 1 && (i & 1));
        const double th = 0.45 + 0.01 * i + 0.003 * r;
        const double c = std::cos(th), s = std::sin(th);
        double* m = k.data() + (((size_t)r * L + i) * n_sub + q) * 8;
        m[0] = c;
        m[6] = c;
        if (y) {
          m[2] = -s;
          m[4] = s;
        } else {
          m[3] = -s;
          m[5] = -s;
        }
      }
  return k;
}

int main(int argc, char** argv) {
  std::map<std::string, std::string> a = {
      {"L", "20"},        {"T", "30"},       {"t_offset", "0"}, {"t_first", "0"},
      {"probe", "-1"},    {"kick", "x"},     {"n_sub", "1"},    {"noise", "depol"},
      {"zsite", "0"},     {"energy", "0"},   {"want_fwd", "1"}, {"want_echo", "1"},
      {"n_pre", "0"},     {"octet", "6"},    {"lightcone", "1"}, {"lc_wide", "1"},
      {"lc_wide3", "1"},  {"dual", "1"},     {"runahead", "1"}, {"wavefront", "1"},
      {"wf_cap", "4"},    {"split13", "0"},  {"mode", "autocorr"}};
  for (int i = 1; i < argc; ++i) {
    const char* eq = std::strchr(argv[i], '=');
    const std::string key(argv[i], eq ? (size_t)(eq - argv[i]) : 0);
    if (!eq || !a.count(key)) return usage("unknown argument");
    a[key] = eq + 1;
  }
  auto num = [&](const char* k) { return std::atoi(a[k].c_str()); };
  const std::string pat = a["kick"], noise = a["noise"];
  if (pat != "x" && pat != "y" && pat != "xy_cycle" && pat != "xy_cycle5" && pat != "gen")
    return usage("bad kick");
  if (noise != "none" && noise != "depol" && noise != "device" && noise != "bond" &&
      noise != "device_bond")
    return usage("bad noise");
  const std::string mode = a["mode"];
  if (mode != "autocorr" && mode != "energy" && mode != "sample") return usage("bad mode");
  const bool autocorr = mode == "autocorr";
  const bool device = noise == "device" || noise == "device_bond";
  const bool bond = noise == "bond" || noise == "device_bond";
  const bool zsite = num("zsite") != 0, energy = num("energy") != 0;
  const int n_pre = num("n_pre");

  // the problem, as check_problem and autocorr_impl's own checks admit it
  dtc_problem pr{};
  pr.L = num("L");
  pr.T = num("T");
  pr.n_inst = 1;
  pr.probe_site = num("probe") < 0 ? pr.L / 2 : num("probe");
  pr.t_offset = num("t_offset");
  pr.n_sub = num("n_sub");
  pr.t_first = num("t_first");
  pr.want_fwd = num("want_fwd");
  pr.want_echo = num("want_echo");
  if (pr.L < 1 || pr.L > 32 || pr.T < 1 || pr.probe_site >= pr.L || pr.t_offset < 0 ||
      pr.t_first < 0 || pr.t_first >= pr.T || pr.n_sub < 1 || pr.n_sub > 8)
    return usage("problem out of range");
  if (bond && pr.t_offset != 0) return usage("bond noise needs t_offset = 0");
  if (energy && (device || bond || zsite || n_pre)) return usage("the energy echo runs alone");
  if (!autocorr && (energy || zsite || n_pre)) return usage("a forward sweep takes no autocorr key");
  if (mode == "sample" && (device || bond)) return usage("sampling runs depolarizing or noiseless");
  if (bond && n_pre) return usage("bond noise runs without a prefix");
  const int P = pr.T - 1 + pr.t_offset;
  if (n_pre < 0 || (n_pre && (zsite || pr.t_first + pr.t_offset <= n_pre || P <= n_pre)))
    return usage("a prefixed run measures the probe, only after the prefix's periods");
  const int n_rows = std::max(1, P);
  const std::vector<double> kick = kick_table(pat, n_rows, pr.L, pr.n_sub);
  std::vector<double> h(pr.L), phi(pr.L);
  for (int i = 0; i < pr.L; ++i) {
    h[i] = 0.3 + 0.07 * i;
    phi[i] = 1.1 - 0.05 * i;
  }
  pr.h = h.data();
  pr.phi = phi.data();
  pr.kick = kick.data();

  SchedOpts so;
  so.lightcone = num("lightcone") != 0;
  so.lc_wide = num("lc_wide") != 0;
  so.lc_wide3 = so.lc_wide && num("lc_wide3") != 0;  // (as dtc_open)
  so.dual = num("dual") != 0;
  so.runahead = num("runahead") != 0;
  so.wavefront = num("wavefront") != 0;
  so.wf_cap = num("wf_cap");
  so.split13 = num("split13") != 0;
  if (so.wf_cap < 2 || so.wf_cap > dtc::kWfSteps) return usage("wf_cap out of range");

  RunCfg rc{};
  rc.prob = &pr;
  rc.n_traj = 1;
  rc.noisy = noise != "none";
  rc.row_kind = classify_rows(&pr);
  rc.pl = autocorr_plan(pr.L, rc.row_kind, so,
                        autocorr && !device && !zsite && !n_pre && !bond && !energy);
  rc.device = device;
  rc.bond = bond;
  rc.octet_bits = num("octet");

  SchedReq rq;
  rq.want_fwd = !energy && pr.want_fwd;
  rq.want_echo = energy || pr.want_echo;
  rq.meas_f = zsite ? dtc::kMeasSites : dtc::kMeasProbe;
  rq.n_obs_f = zsite ? 1 + pr.L : 2;
  rq.energy = energy;
  rq.n_pre = n_pre;
  rq.octet = rc.octet_bits;

  // five fake, distinct buffers (never dereferenced)
  const size_t span = (size_t)1 << 40;
  auto fake = [&](int k) { return (uintptr_t)(k + 1) << 44; };
  const SchedBufs bufs{(const double2*)fake(0), (double2*)fake(1), (double2*)fake(2),
                       (double*)fake(3), (double*)fake(4)};
  const std::vector<DumpRole> roles = {{"F0", bufs.F0, span, 16},         {"F", bufs.F, span, 16},
                                       {"E", bufs.E, span, 16},           {"vals_f", bufs.vals_f, span, 8},
                                       {"vals_e", bufs.vals_e, span, 8}};
  WfTables wt;
  std::vector<Launch> sched;
  SchedInfo info;
  if (!autocorr) {
    // the forward sweeps: F, E and the rows (fake addresses as above)
    const char* err = nullptr;
    if (mode == "energy") err = build_energy_schedule(rc, bufs.F, bufs.vals_f, sched);
    else sched = build_sample_schedule(rc, bufs.F);
    if (err) {
      std::printf("error %s\n", err);
      return 1;
    }
    dump_schedule(stdout, sched, {{"F", bufs.F, span, 16}, {"E", bufs.E, span, 16},
                                  {"vals", bufs.vals_f, span, 8}});
    int shape[6] = {}, t_states = 0, z = 0, xpost = 0, xpre = 0;
    for (const Launch& l : sched) {
      const int s = pass_shape(l.ps);
      if (s >= 0 && s < 6) ++shape[s];
      t_states += l.t_state >= 0;
      z += (l.meas_parts & dtc::kPartZ) != 0;
      xpost += (l.meas_parts & dtc::kPartXPost) != 0;
      xpre += (l.meas_parts & dtc::kPartXPre) != 0;
    }
    std::printf("tally launches=%zu K=%d KD=%d DK=%d KDK=%d D=%d t_state=%d Z=%d XPost=%d XPre=%d\n",
                sched.size(), shape[dtc::kShapeK], shape[dtc::kShapeKD], shape[dtc::kShapeDK],
                shape[dtc::kShapeKDK], shape[dtc::kShapeD], t_states, z, xpost, xpre);
    return 0;
  }
  if (const char* err = build_autocorr_schedule(rc, so, rq, bufs, wt, sched, info)) {
    std::printf("error %s\n", err);
    return 1;
  }
  dump_schedule(stdout, sched, roles);
  std::printf("info dev_ahead=%d n_folds=%d rebuilt=%d groups=%zu tb0=%d\n", (int)info.dev_ahead,
              info.n_folds, (int)info.rebuilt, rc.pl.groups.size(), rc.pl.groups[0].tb);
  for (size_t i = 0; i < wt.keys.size(); ++i) std::printf("wf_set %zu %s\n", i, wt.keys[i].c_str());
  int shape[6] = {}, lc_form[3] = {}, wf_tile[2] = {}, folds = 0;
  for (const Launch& l : sched) {
    folds += l.dst2 != nullptr;
    if (l.wf_steps) {
      ++wf_tile[l.wf_tile];
      continue;
    }
    const int s = pass_shape(l.ps);
    if (s >= 0 && s < 6) ++shape[s];
    if (s == dtc::kShapeLC) ++lc_form[l.ps.lc_wide];
  }
  std::printf("tally launches=%zu K=%d KD=%d DK=%d KDK=%d D=%d LC=%d lc8=%d lc10=%d lc12=%d "
              "folds=%d wf0=%d wf1=%d\n",
              sched.size(), shape[dtc::kShapeK], shape[dtc::kShapeKD], shape[dtc::kShapeDK],
              shape[dtc::kShapeKDK], shape[dtc::kShapeD], shape[dtc::kShapeLC], lc_form[0],
              lc_form[1], lc_form[2], folds, wf_tile[0], wf_tile[1]);
  return 0;
}
