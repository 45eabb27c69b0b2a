"""The batch schedules (csrc/dtc_schedule.h) on the CPU:
tools/schedule_check.cpp builds the schedule of a case exactly as the engine's
autocorr_impl, energy_impl or dtc_sample does and dumps every field of every
launch.  Each case of tests/golden/schedules.json -- the headline line, each
scheduling option off, the wavefront threshold, device-like and bond noise, the
energy echo, per-site Z, a prefix, every plan shape; the energy and sampling
sweeps (mode=energy, mode=sample) -- must give the recorded tally and dump hash,
and every dump must have the structure the engine relies on.  A change that alters
a schedule shows up here first (tools/schedule_golden.py refreshes the file for
one that is meant to).  Built plain and with the host sanitizers; a stand-alone
binary either way."""
import hashlib
import json
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "noise-resilience-in-discrete-time-crystal-realizations-on-quantum-computers_amd"
# the moved code is kept as it was written for the device compiler: its short
# KickDesc initialisers and dtc_rng.h's `#pragma unroll` are not errors here
WARN = ["-Wall", "-Wextra", "-Werror", "-Wno-missing-field-initializers", "-Wno-unknown-pragmas"]
SANITIZE = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
K_SHAPE, KD_SHAPE, KDK_SHAPE, WF_SHAPE = 0, 1, 3, -2
PART_Z, PART_XPOST, PART_XPRE = 1, 2, 4

with open(os.path.join(ROOT, "tests", "golden", "schedules.json")) as _f:
    CASES = json.load(_f)["cases"]


def mode_of(c):
    return dict(tok.split("=", 1) for tok in c["args"]).get("mode", "autocorr")


AUTOCORR_CASES = [c for c in CASES if mode_of(c) == "autocorr"]
ENERGY_CASES = [c for c in CASES if mode_of(c) == "energy"]
SAMPLE_CASES = [c for c in CASES if mode_of(c) == "sample"]


def build(out_dir, flags):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    exe = str(out_dir / "schedule_check")
    subprocess.run([cxx, "-std=c++17", *WARN, "-O1", *flags, "-D__HIP_PLATFORM_AMD__",
                    "-I", os.path.join(rocm, "include"), "-I", os.path.join(ROOT, PKG, "csrc"),
                    os.path.join(ROOT, "tools", "schedule_check.cpp"), "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def dumps(tmp_path_factory):
    """Every case's dump, from the plain build."""
    exe = build(tmp_path_factory.mktemp("schedule"), [])
    out = {}
    for c in CASES:
        r = subprocess.run([exe, *c["args"]], capture_output=True, text=True)
        assert r.returncode == 0, (c["name"], r.stdout[-400:], r.stderr[-400:])
        out[c["name"]] = r.stdout
    return out


def parse(dump):
    """The launches of a dump as dicts (ps / ps2 as dicts of their own)."""
    launches = []
    for line in dump.splitlines():
        if not line.startswith("sched "):
            continue
        d = {}
        for key in ("ps2", "ps"):
            m = re.search(r" %s=\[([^\]]*)\]" % key, line)
            d[key] = dict(tok.split("=", 1) for tok in m.group(1).split())
            line = line[:m.start()] + line[m.end():]
        toks = line.split()
        assert int(toks[1]) == len(launches)
        d.update(tok.split("=", 1) for tok in toks[2:])
        d["shape"] = int(d["shape"])
        d["no_store"] = int(d["no_store"])
        d["meas"] = [int(v) for v in d["meas"].split(",")]
        d["wf"] = [int(v, 16) if i == 2 else int(v) for i, v in enumerate(d["wf"].split(","))]
        d["parts"] = int(d["parts"])
        launches.append(d)
    return launches


def case_args(c):
    a = {"L": "20", "T": "30", "t_offset": "0", "t_first": "0", "noise": "depol", "zsite": "0",
         "energy": "0", "want_fwd": "1", "want_echo": "1", "n_pre": "0"}
    a.update(tok.split("=", 1) for tok in c["args"])
    return a


def offset(ptr, role):
    assert ptr.startswith(role + "+"), (ptr, role)
    return int(ptr[len(role) + 1:])


def test_case_list_covers_the_shipped_configurations():
    names = {c["name"] for c in CASES}
    assert len(names) == len(CASES) >= 30
    assert sum("dump" in c for c in CASES) == 3


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_schedule_matches_golden(dumps, case):
    dump = dumps[case["name"]]
    tally = [ln for ln in dump.splitlines() if ln.startswith("tally ")]
    assert tally == ["tally " + case["tally"]]
    if "dump" in case:
        assert dump.splitlines() == case["dump"]
    assert hashlib.sha256(dump.encode()).hexdigest() == case["sha256"]


@pytest.mark.parametrize("case", AUTOCORR_CASES, ids=[c["name"] for c in AUTOCORR_CASES])
def test_schedule_structure(dumps, case):
    a = case_args(case)
    L, T, t_off, t_first = (int(a[k]) for k in ("L", "T", "t_offset", "t_first"))
    zsite, energy = a["zsite"] == "1", a["energy"] == "1"
    sched = parse(dumps[case["name"]])
    assert sched
    # basis_source sets the basis later; the first launch reads what the engine hands it
    assert all(l["basis"] == "-" for l in sched)
    assert sched[0]["src"] == "F0+0"
    # the echo chains: every launch writes E, and a chain's last launch, and
    # only it, stores nothing; a chain starts in E only behind a dual pass
    open_chain = False
    for l in sched:
        if l["dst"] == "E+0":
            assert open_chain or l["src"] == "F+0", l
            open_chain = not l["no_store"]
        else:
            assert l["dst"] == "F+0" and not l["no_store"] and not open_chain, l
            open_chain = l["dst2"] != "-"
        # a dual pass: a stored K-D-K or K-D whose branch goes to E
        if l["dst2"] != "-":
            assert l["dst2"] == "E+0" and l["shape"] in (KD_SHAPE, KDK_SHAPE) and not l["no_store"], l
        if l["shape"] == WF_SHAPE:
            assert 1 <= l["wf"][0] <= 4, l
    assert not open_chain
    if a["noise"] in ("device", "bond", "device_bond") or zsite or a["n_pre"] != "0":
        assert all(l["shape"] != WF_SHAPE for l in sched)
    # one forward and one echo row per measured time past the initial state
    times = [t for t in range(t_first, T) if t + t_off >= 1]
    n_obs_f = 1 + L if zsite else 2
    fwd_rows = [offset(l["meas_out"], "vals_f") for l in sched
                if l["dst"] == "F+0" and l["meas"][0] != 0]
    want_f = (a["want_fwd"] == "1" and not energy) or zsite
    assert fwd_rows == ([t * n_obs_f for t in times] if want_f else [])
    ends = [l for l in sched if l["no_store"]]
    if energy:
        assert all(l["parts"] & 1 and l["parts"] & 8 for l in ends)
        echo_rows = [offset(l["energy_row"], "vals_e") // (3 * L) for l in ends]
    else:
        assert all(l["meas"][0] == 1 and l["parts"] == 0 for l in ends)
        echo_rows = [offset(l["meas_out"], "vals_e") // 2 for l in ends]
    assert echo_rows == (times if a["want_echo"] == "1" or energy else [])


def site_groups(L):
    """How many site groups make_plan gives L sites: 12 in the low group, then
    up to 9 per further group."""
    return 1 if L <= 12 else 1 + (L - 12 + 8) // 9


@pytest.mark.parametrize("case", ENERGY_CASES, ids=[c["name"] for c in ENERGY_CASES])
def test_energy_schedule_structure(dumps, case):
    """The rules of the energy sweep (the comment of build_energy_schedule), not
    its builder: which launch measures what into which time row."""
    a = case_args(case)
    L, T, t_off = (int(a[k]) for k in ("L", "T", "t_offset"))
    G = site_groups(L)
    sched = parse(dumps[case["name"]])
    times = [t for t in range(T) if t + t_off >= 1]
    assert bool(sched) == (T - 1 + t_off > 0)
    for l in sched:
        assert l["src"] == l["dst"] == "F+0" and l["dst2"] == "-" and l["basis"] == "-", l
        assert l["meas"] == [3 if l["parts"] else 0, 0, 4 * L], l
        assert l["meas_out"] == "-" and int(l["meas_stride"]) == T * 3 * L, l
        assert (l["energy_row"] != "-") == bool(l["parts"] & PART_Z), l
        assert ("row_pre" in l) == bool(l["parts"] & PART_XPRE), l
    z_rows = [offset(l["energy_row"], "vals") for l in sched if l["parts"] & PART_Z]
    assert z_rows == [t * 3 * L for t in times]
    has_d = [l for l in sched if l["ps"]["diag"] != "0"]
    bond = a["noise"] in ("bond", "device_bond")
    for l in sched:
        want = "1,0,%s,0" % l["ps"]["d"] if bond and l in has_d else "0,0,0,0"
        assert l["bond"] == want, l
    if a["noise"] in ("device", "device_bond"):
        # nothing measured across a kick: K-D passes, the closing pass of each
        # measured time takes Z and leaves that time's state
        assert all(l["ps"]["post"] == "-" for l in has_d)
        assert all(("t_state" in l) == bool(l["parts"] & PART_Z) for l in sched)
        assert all(l["parts"] in (0, PART_Z) and not l["no_store"] for l in sched)
        assert [int(l["t_state"]) for l in sched if "t_state" in l] == times
        return
    assert all("t_state" not in l for l in sched)
    # each (time, group) X exactly once: before the post-kick of the pass that
    # closes the time, or at the entry of a later pass on the group
    taken = []
    for l in sched:
        assert not l["parts"] & PART_XPOST or l["parts"] & PART_Z, l
        if l["parts"] & PART_XPOST:
            taken.append((offset(l["energy_row"], "vals") // (3 * L), int(l["ps"]["g"])))
        if l["parts"] & PART_XPRE:
            taken.append((offset(l["row_pre"], "vals") // (3 * L), int(l["ps"]["g"])))
    assert sorted(taken) == [(t, g) for t in times for g in range(G)]
    for i, l in enumerate(sched):
        if l["no_store"]:
            assert i == len(sched) - 1 and l["shape"] == K_SHAPE, l
            assert l["parts"] & PART_XPRE and not l["parts"] & PART_Z, l


@pytest.mark.parametrize("case", SAMPLE_CASES, ids=[c["name"] for c in SAMPLE_CASES])
def test_sample_schedule_structure(dumps, case):
    a = case_args(case)
    T, t_off, t_first = (int(a[k]) for k in ("T", "t_offset", "t_first"))
    sched = parse(dumps[case["name"]])
    assert sched
    for l in sched:
        assert l["src"] == l["dst"] == "F+0" and l["dst2"] == "-" and not l["no_store"], l
        assert l["meas"][0] == 0 and l["parts"] == 0 and l["bond"] == "0,0,0,0", l
        assert "t_state" not in l or l["ps"]["diag"] != "0", l
    assert all(l["ps"]["post"] == "-" for l in sched if l["ps"]["diag"] != "0")
    assert ([int(l["t_state"]) for l in sched if "t_state" in l]
            == list(range(max(t_first, 1 - t_off), T)))


def test_headline_counts_are_exact(dumps):
    """What tests/test_gpu_headline_schedule.py can only bound on the GPU: the
    chains of t = 6 .. 29 end in the 12-site form (24 per batch: that test's
    2 * 23 is a lower bound, t = 6 fits too), t = 5 in the 10-site form,
    t = 2 .. 4 in the 8-site form, and 22 echo chains fold into the forward's
    dual pass."""
    sched = parse(dumps["headline"])
    ends = {}
    for l in sched:
        if l["no_store"] and l["ps"]["lc_w0"] != "-1":
            ends.setdefault(int(l["ps"]["lc_wide"]), []).append(offset(l["meas_out"], "vals_e") // 2)
    assert ends == {2: list(range(6, 30)), 1: [5], 0: [2, 3, 4]}
    assert sum(l["dst2"] != "-" for l in sched) == 22
    info = [ln for ln in dumps["headline"].splitlines() if ln.startswith("info ")]
    assert info == ["info dev_ahead=0 n_folds=22 rebuilt=0 groups=2 tb0=12"]


def test_device_rebuild_cases_rebuild(dumps):
    for name, rebuilt in (("device", 0), ("device_no_runahead", 0), ("device_rebuilt_L12", 1),
                          ("device_rebuilt_zsite_L14", 1)):
        info = [ln for ln in dumps[name].splitlines() if ln.startswith("info ")][0]
        assert "rebuilt=%d" % rebuilt in info, (name, info)
        assert ("dev_ahead=1" in info) == (name == "device"), (name, info)


def test_sanitized_driver_runs_every_case(tmp_path, dumps):
    exe = build(tmp_path, SANITIZE)
    for c in CASES:
        r = subprocess.run([exe, *c["args"]], capture_output=True, text=True)
        assert r.returncode == 0, (c["name"], r.stderr[-2000:])
        assert r.stdout == dumps[c["name"]], c["name"]
