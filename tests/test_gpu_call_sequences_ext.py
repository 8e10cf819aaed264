"""Random call sequences over the entry points that came after tests/test_gpu_call_sequences.py was written - its companion, with another
contract. That file sends legal and illegal arguments to the render path's surface and asks for a return code and an unharmed handle. This one
sends LEGAL calls only (the refusals are the business of the tests/test_*_abi.py files, which need no device) to the ray queries, the radiance,
irradiance, SH, moments, adaptive and visibility gathers, every lightmap call, the irradiance volumes and depth maps and the three moves of a
live scene, host and device route alike, mixed with renders, auxiliary renders, adaptive render sessions, the denoiser, light sampling modes,
the light tables and a change of stream - in seeded random order on one long-lived handle, and asks for the ANSWER of every call: word for word what the numpy
restatement (families that trace nothing) or a fresh handle of the handle's current description that makes only that call (traced families)
answers. The calls, their shapes and their yardsticks are the catalogue of tests/test_gpu_scratch_reuse.py; the pools hold the shapes of that
file and the legal edges: n = 0, a 1 x 1 atlas, 0 passes, an empty mesh, one level, a key base of 0xFFFFFFFF. At the end the handle renders,
after sol_clear, the frame a fresh handle of its final description renders, bit for bit.

The text of every call is appended to a trace file and flushed BEFORE the call is made: what a fault, an abort or a hang leaves behind names the
call, and nothing has to be run again to find it. SOL_TEST_EXT_CALLS / SOL_TEST_EXT_SEED lengthen or shift a campaign (profiles/scratch_reuse.txt
has the lengths that were run); SOL_TEST_EXT_TRACE names a trace file to use instead of the one under pytest's temporary directory.

tests/test_call_sequence_coverage.py reads the keys of CALLS below (one key per distinct call) and ALSO (what a composite call goes through
beside its key): an entry point that takes a SolScene* and is neither here, nor in the older
file, nor excluded there by name with a reason, fails that test."""
import os

import numpy as np
import pytest

import test_gpu_scratch_reuse as S
from solstrale_amd import DeviceScene

pytestmark = pytest.mark.gpu

N_CALLS = int(os.environ.get("SOL_TEST_EXT_CALLS", "150"))  # (a longer campaign: SOL_TEST_EXT_CALLS=1500 SOL_TEST_EXT_SEED=k)
SEED_SHIFT = int(os.environ.get("SOL_TEST_EXT_SEED", "0"))
SEED = S.SEED
U = np.uint32
ATLASES = [(1, 1), (5, 3), (16, 16), (64, 64), (130, 67)]
MESHES = ["empty", "one", "n65", "grid", "lookup", "strip"]
LABELS = ["n0", "n1", "n65", "lookup_mesh", "four_charts", "two_charts", "strip"]
ROWS = [0, 1, 63, 64, 65, 257]
SOME = [1, 63, 64, 65, 257]        # (a lookup takes n = 0 but no null row pointer, and that is what an empty device tensor has)
SAMPLES = [1, 16, 17, 48]
GRIDS = [(1, 1, 1), (2, 3, 4), (5, 5, 5)]
KEY_BASES = [0, 7, 0xFFFFFFFF]


class Fixed:
    """The description of a handle that cannot be moved: the Cornell box, and the light sampling mode in force."""

    def __init__(self):
        self.light = 0

    def key(self):
        return ("cornell", self.light)

    def fresh(self):
        ds = S.cornell()
        if self.light:
            ds.light_sampling(self.light)
        return ds


class Campaign:
    def __init__(self, name, rng):
        self.name, self.rng = name, rng
        self.state = S.Moved() if name == "mesh" else Fixed()
        self.scene = "mesh" if name == "mesh" else "cornell"
        self.ds = DeviceScene(S.dynamic_base(), dynamic_primitives=True) if name == "mesh" else S.cornell()
        self.stream, self.on_own_stream = None, True

    def pick(self, pool):
        return pool[int(self.rng.integers(len(pool)))]

    def flip(self):
        return bool(self.rng.integers(2))

    def atlas(self):
        return self.pick(ATLASES)

    def gather_args(self):
        return dict(scene=self.scene, use_keys=self.flip(), key_base=self.pick(KEY_BASES))


# ---- the calls this file adds to the catalogue: the render path around the newer surface, and what changes the handle ----------------------------
def render(c, entry):
    first, n, seed = c.pick([0, 5]), c.pick(SAMPLES), SEED + int(c.rng.integers(2))

    def run(ds):
        ds.clear()
        ds.render(first, n, seed)
        return ds.read()
    return S.Step(entry, f"clear, render({first}, {n}, {seed}), read", run)


def clear(c, entry):
    def run(ds):
        ds.render(0, 1, SEED)
        ds.clear()
        return ds.read()
    return S.Step(entry, "render, clear, read", run)


def render_aux(c, entry):
    n = c.pick([1, 4, 17])

    def run(ds):
        ds.clear_aux()
        ds.render_aux(0, n, SEED)
        return ds.read_aux()
    return S.Step(entry, f"clear_aux, render_aux(0, {n}), read_aux", run)


def adaptive_session(c, entry):
    rnd, mn, mx, thr = c.pick([(16, 16, 48, 0.05), (16, 32, 64, 0.5)])

    def run(ds):
        ds.adaptive_begin(rnd, mn, mx, thr)
        rounds = ds.adaptive_run(SEED)
        counts, frame = ds.adaptive_counts(), ds.read()
        image = ds.resolve_image()
        rgb = ds.tonemap_rgb8_adaptive(image)
        ds.adaptive_rescale(image)
        scaled = ds.tonemap_rgb8(image, mx)
        ds.clear()  # (ends the session)
        return np.asarray([rounds], dtype=U), counts, frame, rgb, scaled
    return S.Step(entry, f"adaptive session ({rnd}, {mn}, {mx}, {thr}) to its end, counts, read, both tone maps", run)


def denoise(c, entry):
    iterations = c.pick([1, 3])

    def run(ds):
        ds.clear()
        ds.clear_aux()
        ds.render(0, 16, SEED)
        ds.render_aux(0, 4, SEED)
        albedo, normal, m = ds.resolve_aux()
        image = ds.resolve_image()
        rgb = ds.denoise_rgb8(image, 16, albedo, normal, m, iterations=iterations)
        ds.denoise(image, 16, albedo, normal, m, iterations=iterations)
        after = ds.tonemap_rgb8(image, 16)
        ds.clear()
        ds.clear_aux()
        return rgb, after
    return S.Step(entry, f"render 16, render_aux 4, denoise_rgb8 and denoise in place ({iterations} iterations)", run)


def camera_rays(c, keys):
    x0, y0, x1, y1 = c.pick([(0, 0, 32, 32), (3, 5, 20, 9), (31, 31, 32, 32)])
    sample = c.pick([0, 3])
    call = "camera_ray_keys" if keys else "camera_rays"
    return S.Step("sol_" + call, f"({x0}, {y0}, {x1}, {y1}) sample {sample}", lambda ds: getattr(ds, call)(x0, y0, x1, y1, sample, SEED))


def primitive_records(c):
    if c.name != "mesh":
        return None
    kind = c.pick(["sphere", "quad"])

    def run(ds):
        rec, of = ds.primitive_records(kind)
        return rec[np.argsort(of)], np.sort(of)  # (by the caller's index: the device order is each tree's own)
    return S.Step("sol_scene_primitive_records", kind, run)


def effect(entry, text, act):
    """A call that answers nothing and changes the handle (and with it what the later calls must answer)."""
    def run(ds):
        act(ds)
        return ()
    return S.Step(entry, text, run, lambda: ())


def set_stream(c):
    import torch
    to_own = not c.on_own_stream
    if c.stream is None:
        c.stream = torch.cuda.Stream()

    def act(ds):
        ds.set_stream(0 if to_own else c.stream.cuda_stream)
        c.on_own_stream = to_own
    return effect("sol_scene_set_stream", "the handle's own stream" if to_own else "a stream of torch's", act)


def light_sampling(c):
    mode = c.pick([0, 1, 2])

    def act(ds):
        ds.light_sampling(mode)
        c.state.light = mode
    return effect("sol_light_sampling", f"mode {mode}", act)


def light_tables(c):
    """The tables of the power mode and the light tree, which need that mode once: the handle goes there and back to the mode it was in. The
    tree's boxes carry the scene's box pad, and after sol_scene_set_camera that pad keeps the camera's share as creation saw it
    (csrc/sol_geometry.cpp), which a fresh handle of the moved description does not: away from creation's camera the boxes have no yardstick and
    only their count is compared."""
    home = getattr(c.state, "camera", 0) == 0

    def run(ds):
        ds.light_sampling(2)
        q, cdf, total = ds.light_tables()
        nodes, first_leaf, _ = ds.light_tree()
        ds.light_sampling(c.state.light)
        return q, cdf, np.asarray([total], dtype=np.float64).view(U), nodes if home else np.asarray(nodes.shape, dtype=U), np.asarray([first_leaf], dtype=U)
    return S.Step("sol_light_tables", f"power mode, light_tables, light_tree ({'boxes' if home else 'count'}), the mode it was in", run)


def set_camera(c):
    if c.name != "mesh":
        return None
    k = c.pick([0, 1])

    def act(ds):
        ds.set_camera(S.CAMERAS[k])
        c.state.camera = k
    return effect("sol_scene_set_camera", f"camera {k}", act)


def set_triangles(c, h):
    if c.name != "mesh":
        return None
    import torch
    k = c.pick([0, 1, 2, 3])
    rows = np.ascontiguousarray(S.dynamic_rows(k)["triangles"])

    def act(ds):
        ds.set_triangles(rows if h else torch.from_numpy(rows).cuda())
        c.state.triangles = k
    return effect(S.E("sol_scene_set_triangles", h), f"rows {k}", act)


def set_primitives(c):
    if c.name != "mesh":
        return None
    k = c.pick([0, 1, 2, 3])
    kinds = c.pick([("triangles", "spheres", "quads"), ("spheres", "quads")])  # (spheres and quads move together: one set of rows describes both)

    def act(ds):
        ds.set_primitives(**{kind: S.dynamic_rows(k)[kind] for kind in kinds})
        c.state.primitives = k
        if "triangles" in kinds:
            c.state.triangles = k
    return effect("sol_scene_set_primitives", f"rows {k} of {kinds}", act)


def passes_of(c):
    return c.pick([0, 1, 4])


# ---- the table: entry point -> a draw of one call through it (None: not on this handle) ----------------------------------------------------------
CALLS = {
    "sol_query": lambda c: S.query(c.pick(["closest", "occluded"]), c.pick(ROWS), True, c.scene),
    "sol_query_dev": lambda c: S.query(c.pick(["closest", "occluded"]), c.pick(ROWS), False, c.scene),
    "sol_camera_rays": lambda c: camera_rays(c, False),
    "sol_camera_ray_keys": lambda c: camera_rays(c, True),
    "sol_radiance": lambda c: S.radiance(c.pick(ROWS), c.pick(SAMPLES), True, **c.gather_args()),
    "sol_radiance_dev": lambda c: S.radiance(c.pick(ROWS), c.pick(SAMPLES), False, **c.gather_args()),
    "sol_irradiance": lambda c: S.irradiance(c.pick(ROWS), c.pick(SAMPLES), True, mode=c.pick(["cosine", "sphere"]), **c.gather_args()),
    "sol_irradiance_dev": lambda c: S.irradiance(c.pick(ROWS), c.pick(SAMPLES), False, mode=c.pick(["cosine", "sphere"]), **c.gather_args()),
    "sol_irradiance_rays": lambda c: S.irradiance_rays(c.pick(ROWS), c.pick([0, 17]), c.scene),
    "sol_irradiance_sh": lambda c: S.irradiance_sh(c.pick(ROWS), c.pick(SAMPLES), True, **c.gather_args()),
    "sol_irradiance_sh_dev": lambda c: S.irradiance_sh(c.pick(ROWS), c.pick(SAMPLES), False, **c.gather_args()),
    "sol_irradiance_moments": lambda c: S.irradiance_moments(c.pick(ROWS), c.pick(SAMPLES), True, **c.gather_args()),
    "sol_irradiance_moments_dev": lambda c: S.irradiance_moments(c.pick(ROWS), c.pick(SAMPLES), False, **c.gather_args()),
    "sol_irradiance_adaptive": lambda c: S.irradiance_adaptive(c.pick(ROWS), c.pick([16, 17, 48]), 16, c.pick([0.0, 0.05, 0.5]), True, **c.gather_args()),
    "sol_irradiance_adaptive_dev": lambda c: S.irradiance_adaptive(c.pick(ROWS), c.pick([16, 17, 48]), 16, c.pick([0.0, 0.05, 0.5]), False, **c.gather_args()),
    "sol_radiance_rescale": lambda c: S.rescale(c.pick(ROWS), c.pick([1, 16, 48]), True),
    "sol_radiance_rescale_dev": lambda c: S.rescale(c.pick(ROWS), c.pick([1, 16, 48]), False),
    "sol_visibility": lambda c: S.visibility(c.pick(ROWS), c.pick(SAMPLES), c.flip(), True, **c.gather_args()),
    "sol_visibility_dev": lambda c: S.visibility(c.pick(ROWS), c.pick(SAMPLES), c.flip(), False, **c.gather_args()),
    "sol_visibility_oct": lambda c: S.visibility_oct(c.pick(ROWS), c.pick(SAMPLES), c.pick([4, 8]), True, **c.gather_args()),
    "sol_visibility_oct_dev": lambda c: S.visibility_oct(c.pick(ROWS), c.pick(SAMPLES), c.pick([4, 8]), False, **c.gather_args()),
    "sol_lightmap_points": lambda c: S.lm_points(c.pick(MESHES), *c.atlas(), c.flip(), True),
    "sol_lightmap_points_dev": lambda c: S.lm_points(c.pick(MESHES), *c.atlas(), c.flip(), False),
    "sol_lightmap_dilate": lambda c: S.lm_dilate(*c.atlas(), c.pick([3, 27]), passes_of(c), True),
    "sol_lightmap_dilate_dev": lambda c: S.lm_dilate(*c.atlas(), c.pick([3, 27]), passes_of(c), False),
    "sol_lightmap_filter": lambda c: S.lm_filter(*c.atlas(), c.pick([3, 27]), c.pick([1, 3]), True),
    "sol_lightmap_filter_dev": lambda c: S.lm_filter(*c.atlas(), c.pick([3, 27]), c.pick([1, 3]), False),
    "sol_lightmap_filter_var": lambda c: S.lm_filter_var(*c.atlas(), c.pick([1, 3]), True),
    "sol_lightmap_filter_var_dev": lambda c: S.lm_filter_var(*c.atlas(), c.pick([1, 3]), False),
    "sol_lightmap_coords": lambda c: S.lm_coords(c.pick(SOME), True),
    "sol_lightmap_coords_dev": lambda c: S.lm_coords(c.pick(SOME), False),
    "sol_lightmap_sample": lambda c: S.lm_sample(*c.atlas(), c.pick([3, 27]), c.pick([None, 0, 1, 4]), c.pick(ROWS), c.flip(), True),
    "sol_lightmap_sample_dev": lambda c: S.lm_sample(*c.atlas(), c.pick([3, 27]), c.pick([None, 0, 1, 4]), c.pick(SOME), c.flip(), False),
    "sol_lightmap_sh": lambda c: S.lm_sh(*c.atlas(), c.pick([None, 0, 1, 4]), c.pick(SOME), True),
    "sol_lightmap_sh_dev": lambda c: S.lm_sh(*c.atlas(), c.pick([None, 0, 1, 4]), c.pick(SOME), False),
    "sol_lightmap_normals": lambda c: S.lm_normals(c.pick(SOME), True),
    "sol_lightmap_normals_dev": lambda c: S.lm_normals(c.pick(SOME), False),
    "sol_lightmap_mips": lambda c: S.lm_mips(*c.atlas(), c.pick([3, 27]), c.pick([None, 0, 1, 4]), c.pick([None, 1]), True),
    "sol_lightmap_mips_dev": lambda c: S.lm_mips(*c.atlas(), c.pick([3, 27]), c.pick([None, 0, 1, 4]), c.pick([None, 1]), False),
    "sol_lightmap_sample_lod": lambda c: S.lm_sample_lod(*c.atlas(), c.pick([3, 27]), c.pick([None, 4]), c.pick(SOME), True),
    "sol_lightmap_sample_lod_dev": lambda c: S.lm_sample_lod(*c.atlas(), c.pick([3, 27]), c.pick([None, 4]), c.pick(SOME), False),
    "sol_lightmap_lod": lambda c: S.lm_lod(c.pick(SOME), *c.atlas(), True),
    "sol_lightmap_lod_dev": lambda c: S.lm_lod(c.pick(SOME), *c.atlas(), False),
    "sol_lightmap_charts": lambda c: S.lm_charts(c.pick(LABELS), True),
    "sol_lightmap_charts_dev": lambda c: S.lm_charts(c.pick(LABELS), False),
    "sol_lightmap_dilate_charts": lambda c: S.lm_dilate_charts(*c.atlas(), c.pick([3, 27]), passes_of(c), True),
    "sol_lightmap_dilate_charts_dev": lambda c: S.lm_dilate_charts(*c.atlas(), c.pick([3, 27]), passes_of(c), False),
    "sol_lightmap_sample_charts": lambda c: S.lm_sample_charts(*c.atlas(), c.pick([3, 27]), passes_of(c), c.pick(SOME), True),
    "sol_lightmap_sample_charts_dev": lambda c: S.lm_sample_charts(*c.atlas(), c.pick([3, 27]), passes_of(c), c.pick(SOME), False),
    "sol_lightmap_chart_levels": lambda c: S.lm_chart_levels(*c.atlas(), passes_of(c), True),
    "sol_lightmap_chart_levels_dev": lambda c: S.lm_chart_levels(*c.atlas(), passes_of(c), False),
    "sol_volume_points": lambda c: S.vol_points(c.pick(GRIDS), True),
    "sol_volume_points_dev": lambda c: S.vol_points(c.pick(GRIDS), False),
    "sol_volume_build": lambda c: S.vol_build(c.pick(GRIDS), True),
    "sol_volume_build_dev": lambda c: S.vol_build(c.pick(GRIDS), False),
    "sol_volume_sample": lambda c: S.vol_sample(c.pick(GRIDS), c.pick(ROWS), True),
    "sol_volume_sample_dev": lambda c: S.vol_sample(c.pick(GRIDS), c.pick(ROWS), False),
    "sol_volume_build_depth": lambda c: S.vol_build_depth(c.pick(GRIDS), c.pick([4, 8]), True),
    "sol_volume_build_depth_dev": lambda c: S.vol_build_depth(c.pick(GRIDS), c.pick([4, 8]), False),
    "sol_volume_sample_depth": lambda c: S.vol_sample_depth(c.pick(GRIDS), c.pick([4, 8]), c.pick(ROWS), True),
    "sol_volume_sample_depth_dev": lambda c: S.vol_sample_depth(c.pick(GRIDS), c.pick([4, 8]), c.pick(ROWS), False),
    "sol_render": lambda c: render(c, "sol_render"),
    "sol_clear": lambda c: clear(c, "sol_clear"),
    "sol_render_aux": lambda c: render_aux(c, "sol_render_aux"),
    "sol_adaptive_begin": lambda c: adaptive_session(c, "sol_adaptive_begin"),
    "sol_denoise": lambda c: denoise(c, "sol_denoise"),
    "sol_light_tables": light_tables,
    "sol_scene_primitive_records": primitive_records,
    "sol_scene_set_stream": set_stream,
    "sol_light_sampling": light_sampling,
    "sol_scene_set_camera": set_camera,
    "sol_scene_set_triangles": lambda c: set_triangles(c, True),
    "sol_scene_set_triangles_dev": lambda c: set_triangles(c, False),
    "sol_scene_set_primitives": set_primitives,
}
NAMES = sorted(CALLS)
# What a composite call of the table goes through beside the entry point it is listed under (tests/test_call_sequence_coverage.py reads this too).
ALSO = {
    "sol_render": ["sol_read"],
    "sol_adaptive_begin": ["sol_adaptive_round", "sol_adaptive_counts", "sol_tonemap_rgb8_adaptive", "sol_adaptive_rescale"],
    "sol_denoise": ["sol_resolve_aux", "sol_denoise_rgb8"],
    "sol_light_tables": ["sol_light_tree"],
}


def final_frame(ds):
    ds.set_stream(0)
    ds.light_sampling(0)
    ds.clear()
    ds.render(0, 16, SEED)
    return ds.read()


@pytest.mark.timeout(600)
@pytest.mark.parametrize("name", ["cornell", "mesh"])
def test_random_sequences_of_legal_calls_answer_what_each_call_answers_alone(name, tmp_path):
    rng = np.random.default_rng({"cornell": 31, "mesh": 32}[name] + 1000 * SEED_SHIFT)
    c = Campaign(name, rng)
    trace = open(os.environ.get("SOL_TEST_EXT_TRACE") or tmp_path / "calls.txt", "a")
    tally = {}
    try:
        done = 0
        while done < N_CALLS:
            entry = NAMES[int(rng.integers(len(NAMES)))]
            step = CALLS[entry](c)
            if step is None:  # (a move on a handle that was not created for moves)
                continue
            assert step.entry == entry, (step.entry, entry)
            print(f"{name} {done}: {step.text}", file=trace, flush=True)
            got = S.host(step.run(c.ds))
            S.assert_same(got, S.expected(step, c.state.key(), c.state.fresh), (done, step.text, c.state.key()), step.nan_for_nan)
            tally[entry] = tally.get(entry, 0) + 1
            done += 1
        print(f"{name} {done}: the closing frame", file=trace, flush=True)
        got = final_frame(c.ds)
        c.state.light = 0
        with c.state.fresh() as fresh:
            want = final_frame(fresh)
        S.assert_same(got, want, (name, "the closing frame", c.state.key()))
        assert (want != 0).any()
        print(name, dict(sorted(tally.items())))
    finally:
        trace.close()
        c.ds.close()
