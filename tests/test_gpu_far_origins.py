"""The device's fp32 search at far ray origins, scaled directions and ties at the upper end of the interval (rule 1's distance
clause; sol_query / sol_radiance / sol_visibility / sol_scene_set_camera). The rays and the three yardsticks are tests/far_rays.py's: the
double oracle (the truth), the float oracle and a tree-free evaluation of the contract's primitive tests over all primitives. Inside the
envelope (origins up to E_MEASURED x S from the scene; tests/test_far_origins.py measures it on the CPU) every world tree must give the
tree-free answer bit for bit; beyond it the calls must return proper answers, and what differs is recorded (profiles/far_origins.txt) -
lines starting with "far:" are that record. The scene has 113 primitives, batches 1200 rays, frames 32 x 32."""
import contextlib
import os

import numpy as np
import pytest

import far_rays as fr
import orc
from far_rays import CLASSES, E_MEASURED, HIT, INF, LADDER, MISS
from solstrale_amd import AlbedoShader, CameraConfig, DeviceScene, RenderConfig, _abi

pytestmark = pytest.mark.gpu
F = np.float32
INSIDE = [r for r in LADDER if r <= E_MEASURED]
BEYOND = [r for r in LADDER if r > E_MEASURED]
# the default tree, the variants tests/test_gpu_parity.py::test_tree_and_schedule_variants_are_bit_identical sets through the environment, and
# the explicit device build
TREES = {"default": ({}, None), "bvh_ref": ({"SOL_BVH": "ref"}, None), "bvh_sah": ({"SOL_BVH": "sah"}, None), "switch_0": ({"SOL_SWITCH": "0"}, None),
         "switch_40": ({"SOL_SWITCH": "40"}, None), "sah_octant": ({"SOL_BVH": "sah", "SOL_SLOTS": "octant"}, None), "split_0": ({"SOL_SPLIT": "0"}, None),
         "split_100": ({"SOL_SPLIT": "100", "SOL_SPLIT_SLACK": "0"}, None), "tree_device": ({}, _abi.TREE_DEVICE)}
_answers = {}


@contextlib.contextmanager
def tree(name, scene=None):
    """A handle of the ladder's scene (or `scene`) with world tree `name`; the variant's environment holds while the handle lives."""
    env, world_tree = TREES[name]
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        with DeviceScene(scene or fr.ladder_scene(), world_tree=world_tree) as ds:
            yield ds
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def answers(name):
    """{ratio: (closest_hits, occluded)} of every rung's batch on tree `name`, asked once per process."""
    if name not in _answers:
        with tree(name) as ds:
            _answers[name] = {r: (ds.closest_hits(fr.ladder_batch(r)["rays"]), ds.occluded(fr.ladder_batch(r)["rays"])) for r in LADDER}
    return _answers[name]


def bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def differs(a, b):
    """Rows of two SolRayHit arrays that are not the same bytes."""
    return (a.view(np.uint32).reshape(-1, 8) != b.view(np.uint32).reshape(-1, 8)).any(axis=1)


def check_proper(hits, occ, rays, desc):
    """What every answer to a valid ray is, at any distance: HIT or MISS; a miss is (inf, 0, ..); a hit has a finite t inside the ray's own
    interval and names a primitive of the description with its material; occluded says HIT exactly where closest_hits does."""
    assert np.isin(hits["status"], (HIT, MISS)).all()
    assert occ.dtype == np.uint32 and (occ == hits["status"]).all()
    m = hits["status"] == MISS
    assert (hits["t"][m] == INF).all() and (hits["reserved"] == 0).all()
    for f in ("u", "v", "kind", "dfs_index", "material"):
        assert (hits[f][m].view(np.uint32) == 0).all(), f
    h = ~m
    assert np.isfinite(hits["t"][h]).all() and (hits["t"][h] >= rays[h, 3]).all() and (hits["t"][h] <= rays[h, 7]).all()
    for kind, dfs, mat in {(int(x["kind"]), int(x["dfs_index"]), int(x["material"])) for x in hits[h]}:
        assert fr.primitive_exists(desc, kind, dfs, mat), (kind, dfs, mat)


# ---- 1. inside the envelope: every tree gives the tree-free answer ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(TREES))
def test_inside_the_envelope_every_tree_answers_what_no_tree_answers(name):
    desc = fr.ladder_scene().desc
    got = answers(name)
    for ratio in INSIDE:
        b = fr.ladder_batch(ratio)
        hits, occ = got[ratio]
        check_proper(hits, occ, b["rays"], desc)
        bad = differs(hits, b["free"])  # status, t, u, v, kind, dfs_index and material, bit for bit
        assert not bad.any(), (name, ratio, fr.per_class(bad, b["cls"]), b["rays"][bad][:4], hits[bad][:4], b["free"][bad][:4])
        bad = (hits["status"] != b["status32"]) | (bits(hits["t"]) != bits(b["t32"])) | ((hits["status"] == HIT) & (hits["material"] != b["mat32"]))
        assert not bad.any(), (name, ratio, fr.per_class(bad, b["cls"]), b["rays"][bad][:4], hits[bad][:4], b["t32"][bad][:4])
        lost = fr.lost(b["solid"], hits["status"], hits["t"], b["t64"])
        assert not lost.any(), (name, ratio, fr.per_class(lost, b["cls"]), b["rays"][lost][:4], hits[lost][:4])
        assert (hits["status"] == HIT).mean() > 0.9 and len({int(k) for k in hits["kind"][hits["status"] == HIT]}) == 3


# ---- 2. beyond it: proper answers, and a record of what differs ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(TREES))
def test_beyond_the_envelope_answers_stay_proper(name):
    """A record, not a promise: per rung and class the solid rays, those the float oracle and the device lose, and the rays on which the device
    differs from the float oracle (status or t), from the tree-free evaluation (any word) and from the default tree (any word)."""
    desc = fr.ladder_scene().desc
    got, base = answers(name), answers("default")
    for ratio in LADDER:
        b = fr.ladder_batch(ratio)
        hits, occ = got[ratio]
        if ratio in BEYOND:
            check_proper(hits, occ, b["rays"], desc)
        cls = b["cls"]
        lost32 = fr.lost(b["solid"], b["status32"], b["t32"], b["t64"])
        lost_dev = fr.lost(b["solid"], hits["status"], hits["t"], b["t64"])
        vs_oracle = (hits["status"] != b["status32"]) | (bits(hits["t"]) != bits(b["t32"]))
        vs_free, apart = differs(hits, b["free"]), differs(hits, base[ratio][0])
        for k, c in enumerate(CLASSES):
            print(f"far: {ratio:6d} {c:14s} {name:12s} solid {fr.per_class(b['solid'], cls)[k]:4d} lost_oracle {fr.per_class(lost32, cls)[k]:4d} "
                  f"lost_device {fr.per_class(lost_dev, cls)[k]:4d} dev!=oracle {fr.per_class(vs_oracle, cls)[k]:4d} "
                  f"dev!=tree_free {fr.per_class(vs_free, cls)[k]:4d} trees_apart {fr.per_class(apart, cls)[k]:4d}")


# ---- 3. ties at the upper end of the interval ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["default", "bvh_ref"])
def test_a_tie_at_either_end_of_the_interval_stays_inside(name):
    """Every ray of rungs 1, 16 and E_MEASURED that hits at t, asked again over [tmin, t], [tmin, next above t], [tmin, next below t], [t, inf)
    and [next above t, inf): the tree-free evaluation over the same intervals, inclusive at both ends, says what must come back - the same hit
    bits and all for the first, second and fourth, a miss for the third, the next primitive behind it (or a sphere's far side, or a miss)
    for the fifth. wide_node_test culls in units of a distance a millionth beyond the best t so that the first of these stays inside."""
    sc = fr.ladder_scene()
    slack = fr.sphere_slack_of(fr.scene_S(sc.desc))
    counts = {}
    with tree(name) as ds:
        for ratio in sorted({1, 16, E_MEASURED}):
            b = fr.ladder_batch(ratio)
            first = answers(name)[ratio][0]
            h = first["status"] == HIT
            rays, t = b["rays"][h], first["t"][h]
            up, down = np.nextafter(t, INF), np.nextafter(t, F(0))
            for what, col, val, same in (("tmax=t", 7, t, True), ("tmax=above", 7, up, True), ("tmax=below", 7, down, False), ("tmin=t", 3, t, True),
                                         ("tmin=above", 3, up, False)):
                q = rays.copy()
                q[:, col] = val
                got, occ = ds.closest_hits(q), ds.occluded(q)
                want = fr.tree_free_hits(sc, q, slack)
                check_proper(got, occ, q, sc.desc)
                bad = differs(got, want)
                assert not bad.any(), (name, ratio, what, int(bad.sum()), q[bad][:4], got[bad][:4], want[bad][:4])
                if same:
                    assert not differs(got, first[h]).any(), (name, ratio, what)
                elif col == 7:
                    assert (got["status"] == MISS).all(), (name, ratio, what)
                else:
                    assert ((got["status"] == MISS) | (got["t"] > t)).all() and (got["status"] == HIT).any(), (name, ratio, what)
                counts[(ratio, what)] = (len(q), int((got["status"] == HIT).sum()))
    print(f"far: ties {name}: (ratio, interval): (rays, hits) {counts}; differing from the tree-free evaluation: 0")


# ---- 4. direction length -----------------------------------------------------------------------------------------------------------------------
def test_scaling_a_direction_by_a_power_of_two_scales_t_and_nothing_else():
    """d x 2^k with tmin x 2^-k: every operation of the three primitive tests scales by a power of two without rounding while nothing overflows
    or underflows, so status, primitive, u, v and t x 2^k are those of k = 0, bit for bit - unless the node test's t-space slabs lose a box on
    the way. For k < 0 the float oracle, asked with the scaled direction (its entry keeps tmin = 0.001: nothing lies before the unscaled
    tmin), is the yardstick as well."""
    sc = fr.ladder_scene()
    counts = {}
    with tree("default") as ds:
        for ratio in (1, 16):
            b = fr.ladder_batch(ratio)
            base = answers("default")[ratio][0]
            for k in (-20, -8, -1, 8, 20, 30):
                q = b["rays"].copy()
                q[:, 4:7] = np.ldexp(q[:, 4:7], k)
                q[:, 3] = np.ldexp(q[:, 3], -k)
                assert np.isfinite(q[:, :7]).all() and (q[:, 3] > 1e-30).all()
                got, occ = ds.closest_hits(q), ds.occluded(q)
                assert (occ == got["status"]).all() and np.isin(got["status"], (HIT, MISS)).all()
                back = got.copy()
                back["t"] = np.ldexp(got["t"], k)
                bad = differs(back, base)
                assert not bad.any(), (ratio, k, fr.per_class(bad, b["cls"]), q[bad][:4], got[bad][:4], base[bad][:4])
                if k < 0:
                    status, t, mat = fr.oracle_hits(sc, q, orc.ORC_F32, own_interval=False)
                    bad = (got["status"] != status) | (bits(got["t"]) != bits(t)) | ((status == HIT) & (got["material"] != mat))
                    assert not bad.any(), (ratio, k, fr.per_class(bad, b["cls"]), q[bad][:4], got[bad][:4], t[bad][:4])
                counts[(ratio, k)] = int((got["status"] == HIT).sum())
    print(f"far: scaling: hits per (ratio, k), all bit-identical to k = 0: {counts}")


# ---- 5. batch shapes -----------------------------------------------------------------------------------------------------------------------------
def test_batch_shapes_of_far_rays():
    import torch
    rays = np.concatenate([fr.ladder_batch(r)["rays"] for r in (16, 1024)])
    rays = np.ascontiguousarray(rays[np.random.default_rng(3).permutation(len(rays))])
    with tree("default") as ds:
        whole, whole_occ = ds.closest_hits(rays), ds.occluded(rays)
        dev = torch.from_numpy(rays).cuda()
        assert ds.hits_to_numpy(ds.closest_hits(dev)).tobytes() == whole.tobytes()
        assert ds.occluded(dev).cpu().numpy().view(np.uint32).tobytes() == whole_occ.tobytes()
        for n in (1, 63, 64, 65, 257):
            for first in (0, 1000):
                part = rays[first:first + n]
                assert ds.closest_hits(part).tobytes() == whole[first:first + n].tobytes(), (n, first)
                assert ds.occluded(part).tobytes() == whole_occ[first:first + n].tobytes(), (n, first)
                d = dev[first:first + n].contiguous()
                assert ds.hits_to_numpy(ds.closest_hits(d)).tobytes() == whole[first:first + n].tobytes(), (n, first)
                assert ds.occluded(d).cpu().numpy().view(np.uint32).tobytes() == whole_occ[first:first + n].tobytes(), (n, first)
    assert 0 < (whole["status"] == HIT).sum()


# ---- 6. gathers and radiance from far points -----------------------------------------------------------------------------------------------------
def test_visibility_from_far_points_is_the_association_over_its_own_rays():
    """64 points at 16 x S and 64 at 4 x E_MEASURED x S, the normals pointing at the scene: sol_visibility is the association over sol_query's
    answers to sol_irradiance_rays' rays, word for word (tests/test_gpu_visibility.py's restatement). From that far the scene fills a few
    thousandths of a hemisphere and nearly every sample misses; 64 points of the first rung share the batch so that it also sums hits."""
    import test_gpu_visibility as tv
    points = []
    for ratio in (16, 4 * E_MEASURED, 1):
        r = fr.ladder_batch(ratio)["rays"]
        points.append(r[np.random.default_rng(ratio).permutation(len(r))[:64]])
    points = np.concatenate(points)  # (position, tmin, normal = the aimed direction, tmax)
    k = 48
    with tree("default") as ds:
        for mode in ("cosine", "sphere"):
            import torch
            dev_points = torch.from_numpy(points).cuda()
            status, t, dirs = tv.per_sample_answers(ds, dev_points, 0, k, mode=mode)
            assert np.isin(status, (HIT, MISS)).all()
            for distances in (True, False):
                got = ds.visibility_to_numpy(ds.visibility(dev_points, samples=k, first_sample=0, seed=tv.SEED, distances=distances, mode=mode))
                tv.assert_rows_equal(got, tv.restate(status, t, dirs, k, distances), (mode, distances))
                assert (got["hits"] + got["open"] == k).all()
            assert (status[:, 128:] == HIT).any() and (status == MISS).any()
            print(f"far: visibility {mode}: {int((status[:, :128] == HIT).sum())} hits of {status[:, :128].size} gather rays from the 128 far points, "
                  f"{int((status[:, 128:] == HIT).sum())} of {status[:, 128:].size} from the 64 near ones")


def test_radiance_along_far_rays_sees_what_closest_hits_sees():
    """The oracle's debug_path makes its own camera rays, so it cannot be asked about a caller's; under the albedo shader a radiance sample is
    the background exactly where the ray's search misses and a material's colour (none of them the background's) where it hits."""
    sc = fr.far_scene(RenderConfig(32, 32, 1, AlbedoShader()))
    b = fr.ladder_batch(16)
    n = len(b["rays"])
    rays = np.concatenate([b["rays"], b["rays"]])
    rays[n:, 4:7] = -rays[n:, 4:7]  # (the same origins looking away from the scene: misses)
    with tree("default", sc) as ds:
        rgb, count = ds.radiance(rays, samples=1, seed=5)
        hits = ds.closest_hits(rays)
    assert (count == 1).all() and np.isfinite(rgb).all()
    assert not differs(hits[:n], answers("default")[16][0]).any()  # (the shader does not enter a query)
    assert (hits["status"][:n] == b["status32"]).all() and (hits["status"][n:] == MISS).all() and (hits["status"][:n] == HIT).mean() > 0.9
    background = (rgb == np.array([.2, .3, .4], dtype=F)).all(axis=1)
    assert (background == (hits["status"] == MISS)).all(), int((background != (hits["status"] == MISS)).sum())


# ---- 7. a camera moved far away -------------------------------------------------------------------------------------------------------------------
def test_a_camera_moved_far_away():
    """Created at the near camera, moved along +z and +x to 4, 16, 64 and 256 times creation's S with a lens long enough for the cloud of +-8 to
    fill the frame. The moved handle keeps creation's pad, a handle created with that camera has the larger one: whether their answers differ is
    recorded (tests/test_gpu_set_camera.py asserts the equality for its cameras, all beside their scenes). Asserted for both handles: no solid f64 pixel
    ray is lost up to E_MEASURED, counted in creation's S; a 16-spp frame of the moved handle is finite."""
    sc = fr.ladder_scene()
    S = fr.scene_S(sc.desc)
    rc = RenderConfig(32, 32, 16, sc.render_config.shader)
    with tree("default") as moved:
        for axis in (2, 0):
            for ratio in (4, 16, 64, 256):
                look_from = [0., 0., 0.]
                look_from[axis] = ratio * S
                cam = CameraConfig(float(np.degrees(2 * np.arctan(9. / (ratio * S)))), 0., tuple(look_from), (0., 0., 0.), (0., 1., 0.))
                moved.set_camera(cam)
                rays = moved.camera_rays(0, 0, 32, 32, 0, 7).cpu().numpy().reshape(-1, 8)
                got = moved.closest_hits(rays)
                moved.render(0, 16, 7)
                assert np.isfinite(moved.read()).all()
                fresh_sc = fr.far_scene(rc, camera=cam)
                assert fr.scene_S(fresh_sc.desc) == ratio * S
                with DeviceScene(fresh_sc) as fresh:
                    fresh_rays = fresh.camera_rays(0, 0, 32, 32, 0, 7).cpu().numpy().reshape(-1, 8)
                    want = fresh.closest_hits(fresh_rays)
                assert fresh_rays.tobytes() == rays.tobytes()
                s64, t64, _ = fr.oracle_hits(sc, rays, orc.ORC_F64)
                is_solid = fr.solid(s64, t64)
                lost_moved, lost_fresh = fr.lost(is_solid, got["status"], got["t"], t64), fr.lost(is_solid, want["status"], want["t"], t64)
                free = differs(got, fr.tree_free_hits(sc, rays, fr.sphere_slack_of(S)))
                print(f"far: camera {'xyz'[axis]} {ratio:4d}: f64 hits {int((s64 == HIT).sum())} solid {int(is_solid.sum())} of 1024, lost moved {int(lost_moved.sum())} "
                      f"fresh {int(lost_fresh.sum())}, moved != fresh {int(differs(got, want).sum())}, moved != tree-free {int(free.sum())}")
                assert is_solid.sum() >= 50, int(is_solid.sum())  # (the frame does see the scene)
                if ratio <= E_MEASURED:
                    assert not lost_moved.any() and not lost_fresh.any(), (axis, ratio, rays[lost_moved | lost_fresh][:4])
