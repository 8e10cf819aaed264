"""Adaptive irradiance gathers (sol_irradiance_adaptive, sol_radiance_rescale), the part that needs no GPU: the four entry points are
exported, declared, in HIP_SYMBOLS and in INTEGRATION.md; SolGatherAdaptive (24 bytes) and SolGatherAdaptiveStats (40 bytes) have the same size and
offsets from gcc -std=c99 -pedantic and from ctypes; every refusal answers SOL_EINVAL in the stated order, in front of the device check and with
nothing written; the new kernels are gfx950 code of the library and the radiance families keep their instance counts - and the restatement the GPU
tests compare against (tests/irradiance_adaptive_ref.py) has the properties a stop rule and a rescale must have."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import irradiance_adaptive_ref as ar
import lightmap_filter_var_ref as vr
from solstrale_amd import MOMENTS_DTYPE, _abi, device_count

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "solstrale_hip.h")
GATHER_ENTRY_POINTS = ("sol_irradiance_adaptive_dev", "sol_irradiance_adaptive")
RESCALE_ENTRY_POINTS = ("sol_radiance_rescale_dev", "sol_radiance_rescale")
AD, STATS = _abi.SolGatherAdaptive, _abi.SolGatherAdaptiveStats
AD_OFFSETS = {"size": 0, "round": 4, "min_samples": 8, "reserved": 12, "threshold": 16, "floor": 20}
STATS_OFFSETS = {"size": 0, "rounds": 4, "paths": 8, "rows_valid": 16, "rows_converged": 24, "rows_capped": 32}
INF, NAN = float("inf"), float("nan")
F = np.float32


def test_the_entry_points_are_exported_declared_and_documented():
    lib = _abi.load_hip()
    text = open(HEADER).read()
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in GATHER_ENTRY_POINTS + RESCALE_ENTRY_POINTS:
        assert hasattr(lib, name), f"libsolstrale_hip.so does not export {name}"
        assert name in _abi.HIP_SYMBOLS
        assert re.search(r"\b" + name + r"\b", integration), f"INTEGRATION.md does not name {name}"
    for name in GATHER_ENTRY_POINTS:
        assert re.search(r"\bint " + name + r"\(SolScene\* scene, const (void|SolRay)\* points", text), name
        assert len(getattr(lib, name).argtypes) == 8
    for name in RESCALE_ENTRY_POINTS:
        assert re.search(r"\bint " + name + r"\(SolScene\* scene, const (void|SolRadiance)\* rows", text), name
        assert len(getattr(lib, name).argtypes) == 5
    # the _dev form blocks, and the header says so
    assert re.search(r"BLOCKS: one read-back\s+\*?\s*of the active count per round", text)


def test_the_structs_agree_between_gcc_and_ctypes_and_the_header_is_c99(tmp_path):
    assert C.sizeof(AD) == 24 and C.sizeof(STATS) == 40
    assert {n: getattr(AD, n).offset for n, _ in AD._fields_} == AD_OFFSETS
    assert {n: getattr(STATS, n).offset for n, _ in STATS._fields_} == STATS_OFFSETS
    fields = ", ".join(["(unsigned)sizeof(SolGatherAdaptive)"] + [f"(unsigned)offsetof(SolGatherAdaptive, {n})" for n in AD_OFFSETS]
                       + ["(unsigned)sizeof(SolGatherAdaptiveStats)"] + [f"(unsigned)offsetof(SolGatherAdaptiveStats, {n})" for n in STATS_OFFSETS])
    count = 2 + len(AD_OFFSETS) + len(STATS_OFFSETS)
    src = tmp_path / "sizes.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "solstrale_hip.h"\nint main(void) {\n'
                   f'  printf("{"%u " * count}", {fields});\n  return 0;\n}}\n')
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [24] + list(AD_OFFSETS.values()) + [40] + list(STATS_OFFSETS.values())


# ---- the refusals ------------------------------------------------------------------------------------------------------------------------
def _icfg(**kw):
    c = _abi.SolIrradianceConfig(size=C.sizeof(_abi.SolIrradianceConfig), samples=64)
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def _ad(**kw):
    a = AD(size=C.sizeof(AD), round=16, min_samples=32, threshold=0.05, floor=0.0)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_every_gather_refusal_comes_in_the_stated_order_before_the_device():
    """With or without a GPU. A zeroed block stands in for a scene: its has_medium byte is 0, and nothing else in front of the device check reads the
    handle (tests/test_gpu_irradiance_adaptive.py adds the refusal of a scene with a constant medium, which sits between n == 0 and the null
    pointers). Each bad argument is paired with every LATER one; the earlier one must be named."""
    lib = _abi.load_hip()
    err = lib.sol_last_error
    points, out = (_abi.SolRay * 2)(), (_abi.SolMoments * 2)()
    stand_in = C.create_string_buffer(1 << 20)
    good = dict(scene=stand_in, n=2, c={}, a={}, s={}, points=points, out=out)
    steps = [(dict(scene=None), b"null scene"), (dict(cfg_null=True), b"null configuration"), (dict(c=dict(size=28)), b"SolIrradianceConfig.size"),
             (dict(c=dict(samples=0)), b"samples is 0"), (dict(c=dict(first_sample=0xFFFFFFF0)), b"first_sample"), (dict(n=(1 << 31) + 1), b"2^31"),
             (dict(c=dict(mode=2)), b"unknown mode"),
             (dict(ad_null=True), b"null adaptive configuration"), (dict(a=dict(size=20)), b"SolGatherAdaptive.size"), (dict(a=dict(reserved=1)), b"reserved"),
             (dict(a=dict(round=0)), b"round is 0"), (dict(a=dict(round=24)), b"round is 24"), (dict(a=dict(min_samples=8)), b"min_samples"),
             (dict(a=dict(threshold=NAN)), b"threshold"), (dict(a=dict(threshold=-0.5)), b"threshold"), (dict(a=dict(threshold=INF)), b"threshold"),
             (dict(a=dict(floor=NAN)), b"floor"), (dict(a=dict(floor=-1.0)), b"floor"), (dict(a=dict(floor=INF)), b"floor"),
             (dict(s=dict(size=32)), b"SolGatherAdaptiveStats.size"),
             (dict(points=None), b"null point"), (dict(out=None), b"null output")]
    stats_seen = []
    for name in GATHER_ENTRY_POINTS:
        fn = getattr(lib, name)

        def call(a):
            cfg = None if a.get("cfg_null") else C.byref(_icfg(**a["c"]))
            ad = None if a.get("ad_null") else C.byref(_ad(**a["a"]))
            st = STATS(size=a["s"].get("size", C.sizeof(STATS)), rounds=77, paths=77)
            stats_seen.append(st)
            return fn(a["scene"], a["points"], None, a["n"], cfg, ad, a["out"], C.byref(st))

        def merged(*parts):
            m = dict(good)
            for p in parts:
                for k, v in p.items():
                    m[k] = {**m[k], **v} if k in ("c", "a", "s") else v
            return m

        for k, (broken, word) in enumerate(steps):
            assert call(merged(broken)) == _abi.SOL_EINVAL, (name, word)
            assert word in err() and name.encode() + b":" in err(), (name, word, err())
            for later, later_word in steps[k + 1:]:
                same = (set(later) & set(broken)) - {"c", "a", "s"} or any(set(later.get(g, {})) & set(broken.get(g, {})) for g in ("c", "a", "s"))
                if same or ("cfg_null" in broken and "c" in later) or ("ad_null" in broken and "a" in later):
                    continue  # (two ways to break the same argument)
                assert call(merged(later, broken)) == _abi.SOL_EINVAL and word in err(), (name, word, later, err())
        # n == 0 is SOL_OK on any scene: nothing is read behind the scene pointer and nothing is written, whatever the pointers are - but only
        # behind every refusal of the configurations
        assert call(merged(dict(n=0))) == _abi.SOL_OK and call(merged(dict(n=0, points=None, out=None))) == _abi.SOL_OK, name
        assert fn(stand_in, None, None, 0, C.byref(_icfg()), C.byref(_ad()), None, None) == _abi.SOL_OK  # (stats may be null)
        assert call(merged(dict(n=0, scene=None))) == _abi.SOL_EINVAL and b"null scene" in err()
        assert call(merged(dict(n=0, a=dict(round=8)))) == _abi.SOL_EINVAL and b"round" in err()
        assert call(merged(dict(n=0, s=dict(size=8)))) == _abi.SOL_EINVAL and b"SolGatherAdaptiveStats" in err()
        if device_count() == 0:
            assert call(good) == _abi.SOL_EDEVICE
            assert call(merged(dict(c=dict(mode=_abi.SOL_IRRADIANCE_SPHERE, samples=17, first_sample=5), a=dict(threshold=0.0, floor=2.0, min_samples=0, round=32)))) == _abi.SOL_EDEVICE
    assert bytes(out) == bytes(64)  # nothing was written
    assert all(st.rounds in (0, 77) and st.paths in (0, 77) for st in stats_seen)  # (0: a call with n == 0 that succeeded)


def test_the_rescale_refusals_come_before_the_device():
    lib = _abi.load_hip()
    err = lib.sol_last_error
    rows, out = (C.c_float * 8)(), (C.c_float * 8)()
    stand_in = C.create_string_buffer(1 << 20)
    for name in RESCALE_ENTRY_POINTS:
        fn = getattr(lib, name)
        assert fn(None, rows, 2, 0, None) == _abi.SOL_EINVAL and b"null scene" in err() and name.encode() + b":" in err()
        assert fn(stand_in, None, 2, 0, None) == _abi.SOL_EINVAL and b"target_samples" in err()
        assert fn(stand_in, None, 2, 4, None) == _abi.SOL_EINVAL and b"null row" in err()
        assert fn(stand_in, rows, 2, 4, None) == _abi.SOL_EINVAL and b"null output" in err()
        assert fn(stand_in, None, 0, 4, None) == _abi.SOL_OK  # nothing to do
        assert fn(stand_in, None, 0, 0, None) == _abi.SOL_EINVAL
        if device_count() == 0:
            assert fn(stand_in, rows, 2, 4, out) == _abi.SOL_EDEVICE and fn(stand_in, rows, 2, 4, rows) == _abi.SOL_EDEVICE
    assert bytes(out) == bytes(32)


def test_the_kernels_are_gfx950_code_of_the_library_and_the_radiance_families_keep_their_counts():
    data = open(_abi.HIP_LIB, "rb").read()
    assert b"amdgcn-amd-amdhsa--gfx950" in data
    for kernel in (b"sol_gather_judge_kernel", b"sol_gather_scan_kernel", b"sol_gather_scatter_kernel", b"sol_gather_writeback_kernel",
                   b"sol_rescale_rows_kernel", b"sol_moments_project_kernel"):
        assert kernel in data, kernel
    # the rounds run the ten per-sample instances as they stand: no new instance of any radiance family
    each = set(re.findall(rb"_Z24sol_radiance_each_kernelILb[01]ELb[01]ELb[01]ELb[01]EE", data))
    gather = set(re.findall(rb"_Z19sol_radiance_kernelILb[01]ELb[01]ELb[01]ELb[01]ELb1EE", data))
    plain = set(re.findall(rb"_Z19sol_radiance_kernelILb[01]ELb[01]ELb[01]ELb[01]ELb0EE", data))
    assert (len(each), len(gather), len(plain)) == (10, 10, 10), (sorted(each), sorted(gather), sorted(plain))
    names = set(re.findall(rb"_Z\d+sol_radiance_[a-z_]*kernel\w*", data))
    assert len(names) == 30 + 1, sorted(names)  # (+ sol_radiance_resolve_kernel; the rescale's kernel, sol_rescale_rows_kernel, is no member of the family)


# ---- the restatement's own properties ----------------------------------------------------------------------------------------------------
def _samples(seed, k, n):
    """[k, n, 3] heavy-tailed positive colours."""
    rng = np.random.default_rng(seed)
    return (rng.uniform(0.0, 1.0, (k, n, 3)) ** 4 * 30.0).astype(F)


def _rows_at(colours, valid=None):
    def rows(N):
        with np.errstate(over="ignore", invalid="ignore"):  # (some tests feed colours whose squares overflow, on purpose)
            return vr.moments_of_samples(colours[:N], valid=valid)
    return rows


def test_a_threshold_of_zero_never_stops_a_row_before_the_maximum():
    c = _samples(1, 80, 200)
    c[:, :20] = F(0.5)  # (rows of identical samples, v = 0: even they go on)
    for mx, rnd in ((80, 16), (64, 32), (17, 16), (16, 16), (48, 16)):
        counts, verdicts, rounds = ar.count_map(_rows_at(c), np.ones(200, bool), mx, rnd, 0, 0.0, 0.0)
        assert (counts == mx).all() and (verdicts == ar.CAPPED).all() and rounds == len(ar.round_counts(mx, rnd))
        assert ar.stats_of(counts, verdicts, rounds) == {"rounds": rounds, "paths": 200 * mx, "rows_valid": 200, "rows_converged": 0, "rows_capped": 200}


def test_rows_of_identical_samples_stop_at_the_first_judged_count():
    """Every sample of a row is the same power of two c: sum = N c, sum2 = N c^2 and x = c exactly for N = 16, 32, 48 (N c has at most six
    significant bits), so (sum2 / N) - (x * x) = 0, v = 0 <= t * t for any threshold > 0 - also with a floor above the mean, and with x = 0."""
    c = np.zeros((96, 6, 3), F)
    c[:, 0], c[:, 1], c[:, 2], c[:, 3], c[:, 4] = 0.5, 2.0, 0.125, (0.25, 4.0, 1.0), 0.0
    c[:, 5] = _samples(3, 96, 1)[:, 0]  # (and a noisy row that does not)
    for min_samples, first in ((0, 16), (16, 16), (32, 32), (48, 48)):
        for floor in (0.0, 8.0):
            counts, verdicts, _ = ar.count_map(_rows_at(c), np.ones(6, bool), 96, 16, min_samples, 1e-6, floor)
            assert (counts[:5] == first).all() and (verdicts[:5] == ar.CONVERGED).all(), (min_samples, floor, counts)
            assert counts[5] == 96 and verdicts[5] == ar.CAPPED
    # a single sample per judgement cannot converge: N >= 2 (round 16 makes N = 1 impossible on the device; the rule still says so)
    one = vr.moments_of_samples(c[:1])
    assert (ar.judge(one, 96, 0, 0.5, 0.0) == ar.ACTIVE).all()


def test_a_sum_that_is_not_finite_stops_at_once_and_is_neither_converged_nor_capped():
    c = _samples(5, 64, 8)
    c[3, 1, 0], c[20, 2, 1], c[5, 4, 2] = np.inf, np.nan, F(3e38)  # (3e38: the sum of squares overflows)
    c[40, 6, 1] = -np.inf
    counts, verdicts, rounds = ar.count_map(_rows_at(c), np.ones(8, bool), 64, 16, 32, 0.0, 0.0)
    assert counts.tolist() == [64, 16, 32, 64, 16, 64, 48, 64], counts
    assert (verdicts[[1, 2, 4, 6]] == ar.BROKEN).all() and (verdicts[[0, 3, 5, 7]] == ar.CAPPED).all()
    s = ar.stats_of(counts, verdicts, rounds)
    assert s["rows_capped"] == 4 and s["rows_converged"] == 0 and s["rows_valid"] == 8 and s["paths"] == int(counts.sum())
    # at the maximum a broken row is still broken: the first condition that holds names the reason
    c[60, 0, 0] = np.inf
    counts, verdicts, _ = ar.count_map(_rows_at(c), np.ones(8, bool), 64, 16, 32, 0.0, 0.0)
    assert counts[0] == 64 and verdicts[0] == ar.BROKEN
    # and a row that is not valid has no count at all
    valid = np.array([True, False] * 4)
    counts, verdicts, _ = ar.count_map(_rows_at(_samples(6, 64, 8), valid), valid, 64, 16, 32, 0.0, 0.0)
    assert (counts[~valid] == 0).all() and (counts[valid] == 64).all()


def test_scaling_every_sample_and_the_floor_by_a_power_of_two_leaves_the_count_map_unchanged():
    """c_s -> 2^k c_s: the sums scale by 2^k, the squared sums by 4^k, and with floor -> 2^k floor so do x, the clamp and t; v and t * t scale by 4^k.
    Scaling by a power of two commutes with fp32 rounding while nothing leaves the normal range (1e-3 .. 3e3 before scaling, |k| <= 8), so every
    comparison v <= t * t has the same outcome."""
    c = _samples(8, 96, 300)
    valid = np.ones(300, bool)
    threshold, floor = 0.2, 0.75
    base, verdicts, _ = ar.count_map(_rows_at(c), valid, 64, 16, 32, threshold, floor)
    # (the map is worth comparing: rows stop at 32, at 48 and at the maximum, a fifth of them converged)
    assert len(np.unique(base)) == 3 and (base < 64).sum() >= 30 and (base == 64).sum() >= 30, np.unique(base, return_counts=True)
    assert (verdicts[base < 64] == ar.CONVERGED).all() and (verdicts[base == 64] == ar.CAPPED).all()
    for k in (-8, -3, 1, 5, 8):
        scaled, _, _ = ar.count_map(_rows_at(c * F(2.0 ** k)), valid, 64, 16, 32, threshold, floor * 2.0 ** k)
        assert (scaled == base).all(), k
    # the floor matters: relative to a floor above every mean fewer samples are needed
    floored, _, _ = ar.count_map(_rows_at(c), valid, 64, 16, 32, threshold, 100.0)
    assert (floored <= base).all() and (floored < base).any()


def test_the_rescale_returns_equal_counts_bit_for_bit_and_copies_rows_without_samples():
    rng = np.random.default_rng(11)
    n = 500
    rows = np.zeros((n, 4), F)
    rows[:, :3] = (rng.uniform(0, 1, (n, 3)) ** 6 * 1e4).astype(F)
    rows[:5, :3] = F(3e38), F(-0.0), F(1e-42)  # near overflow, a signed zero, a subnormal
    cnt = rows.view(np.uint32)[:, 3]
    for target in (1, 48, 64, (1 << 24) + 1, 0xFFFFFFEF):
        cnt[:] = target
        assert (ar.rescale(rows, target).view(np.uint32) == rows.view(np.uint32)).all(), target
    # count 0: copied, whatever the words are; elsewhere one rounding of the exact quotient (the float64 steps add 2^-52)
    rows[:5, :3] = F(1.0)
    cnt[:] = rng.integers(1, 200, n)
    cnt[::7] = 0
    rows[::7, :3] = F(123.0)
    out = ar.rescale(rows, 64)
    assert (out.view(np.uint32)[::7] == rows.view(np.uint32)[::7]).all()
    live = cnt != 0
    assert (out.view(np.uint32)[live, 3] == 64).all()
    want = rows[live, :3].astype(np.float64) * 64 / cnt[live, None]
    assert np.abs(out[live, :3] / want - 1).max() <= 2.0 ** -24 + 2.0 ** -50
    # counts above 2^24 are not representable in float32: the step is taken in float64
    big = np.zeros((1, 4), F)
    big[0, :3] = 3.0
    big.view(np.uint32)[0, 3] = (1 << 24) + 1
    assert ar.rescale(big, 1 << 25)[0, 0] == F(3.0 * (1 << 25) / ((1 << 24) + 1)) and ar.rescale(big, 1 << 25).view(np.uint32)[0, 3] == 1 << 25


def test_the_moments_layout_the_rule_reads():
    rows = np.zeros(1, MOMENTS_DTYPE)
    rows["sum"], rows["sum2"], rows["samples"] = (32.0, 32.0, 32.0), (40.0, 40.0, 40.0), 32
    # x = 1, v = (40/32 - 1) / 31 = 0.25 / 31 = 0.0080645: converged at threshold 0.09 (t^2 = 0.0081), not at 0.0898 (t^2 = 0.008064)
    assert ar.judge(rows, 64, 32, 0.09, 0.0)[0] == ar.CONVERGED and ar.judge(rows, 64, 32, 0.0898, 0.0)[0] == ar.ACTIVE
    assert ar.judge(rows, 64, 48, 0.09, 0.0)[0] == ar.ACTIVE and ar.judge(rows, 32, 48, 0.0, 0.0)[0] == ar.CAPPED
    assert ar.judge(rows, 64, 32, 0.0898, 1.01)[0] == ar.CONVERGED  # t = 0.0898 x 1.01: t^2 = 0.008226
