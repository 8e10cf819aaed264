"""The stop rule of the adaptive irradiance gathers and the rescale of sol_radiance_rescale (include/solstrale_hip.h), restated in
numpy: csrc/sol_gather_adaptive.h operation by operation in float32 - every operation rounded once, no fused multiply-add, no square root -, and the
rescale's one step in float64. The estimators are Prepare's (tests/lightmap_filter_var_ref.py). What the device answers is compared with these:
the count maps and the rescaled words bit for bit."""
import numpy as np

import lightmap_filter_var_ref as vr

F = np.float32
ACTIVE, BROKEN, CAPPED, CONVERGED = 0, 1, 2, 3


def judge(moments, max_samples, min_samples, threshold, floor):
    """[n] verdicts of rows that hold samples (MOMENTS_DTYPE or [n, 8] float32 rows whose count is >= 1): the first condition that holds - a sum
    that is not finite (BROKEN), the count at the maximum (CAPPED), the variance of the mean within the tolerance in every channel (CONVERGED)
    - or ACTIVE."""
    w = vr.moments_rows(moments)
    f = w.view(F)
    count = w[:, 3]
    s, q = f[:, 0:3], f[:, 4:7]
    threshold, floor = F(threshold), F(floor)
    with np.errstate(all="ignore"):
        N = count.astype(F)[:, None]
        M = (count - np.uint32(1)).astype(F)[:, None]
        x = s / N
        d = (q / N) - (x * x)
        v = np.where(d > 0, d, F(0)).astype(F) / M
        t = threshold * np.where(x > floor, x, floor).astype(F)
        within = (v <= (t * t)).all(axis=1)
    finite = np.isfinite(s).all(axis=1) & np.isfinite(q).all(axis=1)
    judged = (threshold > 0) & (count >= np.uint32(min_samples)) & (count >= 2)
    out = np.full(len(w), ACTIVE)
    out[judged & within] = CONVERGED
    out[count == np.uint32(max_samples)] = CAPPED
    out[~finite] = BROKEN
    return out


def round_counts(max_samples, round_samples):
    """The counts at which a row is judged: round, 2 round, .., clipped to the maximum."""
    return [min(k * round_samples, max_samples) for k in range(1, -(-max_samples // round_samples) + 1)]


def count_map(rows_at, valid, max_samples, round_samples, min_samples, threshold, floor):
    """The final count of every row and why it stopped. rows_at(N): the fixed call's rows (all points) with samples = N. A row that is not valid
    has count 0. Returns (counts [n] uint32, verdicts [n], rounds)."""
    n = len(valid)
    counts = np.zeros(n, np.uint32)
    verdicts = np.full(n, ACTIVE)
    active = np.asarray(valid, bool).copy()
    rounds = 0
    for N in round_counts(max_samples, round_samples):
        if not active.any() and rounds > 0:
            break
        rounds += 1
        if not active.any():
            break
        v = judge(rows_at(N)[active], max_samples, min_samples, threshold, floor)
        idx = np.flatnonzero(active)
        stop = v != ACTIVE
        counts[idx[stop]] = N
        verdicts[idx[stop]] = v[stop]
        active[idx[stop]] = False
    assert not active.any()
    return counts, verdicts, rounds


def stats_of(counts, verdicts, rounds):
    return {"rounds": rounds, "paths": int(counts.astype(np.uint64).sum()), "rows_valid": int((counts > 0).sum()),
            "rows_converged": int((verdicts == CONVERGED).sum()), "rows_capped": int((verdicts == CAPPED).sum())}


def rescale(rows, target_samples):
    """[n, 4] float32 rows (r, g, b, the bits of the count) -> the same brought to target_samples: float32((float64(word) * target) / count); a row
    with count 0 is copied."""
    a = np.ascontiguousarray(rows, dtype=F).copy()
    count = a.view(np.uint32)[:, 3].copy()
    has = count != 0
    with np.errstate(all="ignore"):
        scaled = ((a[:, :3].astype(np.float64) * np.float64(target_samples)) / np.where(has, count, 1).astype(np.float64)[:, None]).astype(F)
    a[has, :3] = scaled[has]
    a.view(np.uint32)[has, 3] = np.uint32(target_samples)
    return a
