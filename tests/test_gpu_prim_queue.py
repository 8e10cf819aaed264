"""The primitive queue of the search step (sol_trace.h, trav_step_wave<.., QUEUE>; SOL_PRIM_QUEUE): the plain instances of sol_render_kernel
let a lane hold two primitive groups and go on visiting nodes; MEDIUM instances, the query, radiance and visibility kernels keep one group.
The closest hit does not depend on the order of the primitive tests, so every frame must be the float oracle's (parity_util's route, the
allowance of tests/test_gpu_parity.py: no pixel outside 1e-5), single-hit frames and frames of the same scene from kernels of the other
depth bit for bit.
  - two groups held at once: a narrow stack of thin parallel triangles seen through the stack, from both ends and from inside
  - exact ties between groups: coincident triangles in different leaves, reached in both orders - the later dfs wins
  - mixed leaves: triangles, a quad and a sphere under one root, a quad light (the per-group leaf kind)
  - the instances that keep depth 1 (a constant medium) and the needle rule's restart; a query and a radiance call after a render
  - a frame stays a pure function of scene and seed: sample-range split and tile partition"""
import numpy as np
import pytest

import orc
import parity_util as pu
from solstrale_amd import AlbedoShader, CameraConfig, DeviceScene, PathTracingShader, RenderConfig, SceneBuilder, scenes

pytestmark = pytest.mark.gpu
N_STACK = 48


def _colour(k, n):
    return (0.15 + 0.8 * k / n, 0.9 - 0.7 * ((k * 7) % n) / n, 0.2 + 0.6 * ((k * 13) % n) / n)


def stack_scene(look_from, look_at, shader, w=48, h=48, spp=16, mirror=1.0):
    """N_STACK thin parallel triangles, 0.05 apart along z (a stack 2.35 deep, 2.4 wide), each of its own colour and slightly shifted so that
    no two share a coordinate; a quad light beside the stack. A ray along z crosses every triangle's box: consecutive nodes on its way each
    carry hit leaf slots."""
    b = SceneBuilder()
    world = []
    for k in range(N_STACK):
        z = mirror * (0.05 * k + 0.0007 * (k % 5))
        dx, dy = 0.011 * (k % 7) - 0.03, 0.013 * (k % 3) - 0.01
        world.append(b.Triangle((-1.2 + dx, -1.0 + dy, z), (1.2 + dx, -1.0 + dy, z), (0.0 + dx, 1.3 + dy, z), b.Lambertian(b.SolidColor(*_colour(k, N_STACK)))))
    world.append(b.Quad((-3., 2.5, -1.), (6., 0., 0.), (0., 0., 4.), b.DiffuseLight(5., 5., 5.)))
    cam = CameraConfig(40., 0., look_from, look_at, (0., 1., 0.))
    return b.finish(b.Bvh(world), cam, (.3, .4, .5), RenderConfig(w, h, spp, shader))


def _render(sc, spp, counted=False):
    with DeviceScene(sc) as ds:
        ds.render(0, spp, pu.SEED, counted=counted)
        img = ds.read()
        st = ds.stats() if counted else None
        info = ds.info()
    return img, st, info


def _assert_parity(sc, spp, img=None):
    if img is None:
        img, _, _ = _render(sc, spp)
    ref, _ = orc.render(sc, 0, spp, pu.SEED, real=orc.ORC_F32)
    res = pu.compare(img, ref, spp)
    print(res)
    assert np.isfinite(img).all()
    assert res["bad_pixels"] == 0 and res["max_rel"] <= pu.REL_TOL and res["rmse_mean_good"] < 1e-5, res
    return ref


MID_Z = 0.05 * (N_STACK // 2) + 0.02  # (between two triangles of the stack)
# (from inside: the eye stands between two triangles, on the slanted edge of the stack - the triangles are shifted against each other, so the
# rays along z meet the next triangle or pass it and meet a later one)
CAMERAS = {"front": ((0.05, 0.1, -3.0), (0., 0., 1.)), "back": ((-0.04, 0.05, 5.5), (0., 0.1, 1.)),
           "inside": ((0.6, 0.15, MID_Z), (0.62, 0.16, MID_Z + 3.)), "inside_back": ((0.6, 0.15, MID_Z), (0.58, 0.14, MID_Z - 3.))}


@pytest.mark.parametrize("cam", sorted(CAMERAS))
def test_two_groups_held_at_once(cam):
    """Albedo frames (one search per sample, a sum of the hit triangles' own colours) must be the oracle's bit for bit; path-traced frames
    are held to parity_util's bound. The counted render tests at least two triangles per ray: the groups of consecutive nodes."""
    look_from, look_at = CAMERAS[cam]
    sc = stack_scene(look_from, look_at, AlbedoShader())
    img, st, _ = _render(sc, 16, counted=True)
    ref, _ = orc.render(sc, 0, 16, pu.SEED, real=orc.ORC_F32)
    differing = int((img.astype(np.float64) != ref).any(axis=-1).sum())
    print(cam, "albedo pixels differing from the oracle:", differing, "triangle tests per ray:", st["triangle_tests"] / st["rays"])
    assert differing == 0
    assert len(np.unique(img.reshape(-1, 3), axis=0)) > 2  # (several triangles are in view)
    assert st["triangle_tests"] >= 2 * st["rays"], st
    with DeviceScene(sc) as ds:  # the uncounted instance: the same frame
        ds.render(0, 16, pu.SEED)
        assert (ds.read() == img).all()
    _assert_parity(stack_scene(look_from, look_at, PathTracingShader(8)), 16)


@pytest.mark.parametrize("mirror", [1.0, -1.0], ids=["scene", "mirrored"])
@pytest.mark.parametrize("side", [1.0, -1.0], ids=["camera_front", "camera_behind"])
@pytest.mark.parametrize("n_copies", [2, 9])
def test_exact_ties_between_groups(n_copies, side, mirror, monkeypatch):
    """Coincident triangles of different colours: t is equal, the later one in depth-first leaf order wins (bvh.rs:172-178). Two copies in
    different sub-trees of the reference's own topology, far apart in leaf order; nine copies - more than the seven slots of a wide node -
    lie in different leaves whatever the builder does. Camera on either side, scene mirrored: both orders of reaching them."""
    monkeypatch.setenv("SOL_BVH", "ref")
    b = SceneBuilder()
    cols = [(1., 0., 0.)] + [(0.1 * k, 0.3, 1. - 0.1 * k) for k in range(1, n_copies - 1)] + [(.9, .9, .9)]
    tri = lambda c: b.Triangle((-2., -1.5, 0.), (2., -1.5, 0.), (0., 2., 0.), b.Lambertian(b.SolidColor(*c)))
    filler = lambda k: b.Triangle((-3. + 0.5 * k, -2., mirror * (1. + 0.1 * k)), (-2.5 + 0.5 * k, -2., mirror * (1. + 0.1 * k)),
                                  (-2.75 + 0.5 * k, -1.7, mirror * (1.05 + 0.1 * k)), b.Lambertian(b.SolidColor(.2, .8, .2)))
    groups = [b.Bvh([tri(c)] + [filler(4 * i + j) for j in range(3)]) for i, c in enumerate(cols)]
    world = groups + [b.Sphere((0., 50., 0.), 10., b.DiffuseLight(5, 5, 5))]
    cam = CameraConfig(50., 0., (0.3, 0.2, side * 5.), (0., 0., 0.), (0, 1, 0))
    sc = b.finish(b.Bvh(world), cam, (.1, .1, .1), RenderConfig(64, 48, 16, AlbedoShader()))
    img, _, _ = _render(sc, 16)
    ref = _assert_parity(sc, 16, img)
    want = np.array(cols[-1], dtype=np.float32) * 16
    inside = np.abs(ref - want.astype(np.float64)).max(axis=-1) < 1e-5  # pixels whose samples all hit the coincident triangles
    assert inside.sum() > 300 and np.allclose(img[inside], want, atol=1e-5)
    for c in cols[:-1]:  # an earlier copy's colour shows nowhere
        assert not (np.abs(img - np.array(c, dtype=np.float32) * 16).max(axis=-1) < 1e-5).any(), c
    sc2 = b.finish(b.Bvh(world), cam, (.1, .1, .1), RenderConfig(64, 48, 16, PathTracingShader(8)))
    _assert_parity(sc2, 16)


def test_mixed_leaves():
    """Triangles, a quad and a sphere under one root: nodes that list references beside triangle leaves; each held group has its own kind."""
    b = SceneBuilder()
    grey, blue = b.Lambertian(b.SolidColor(.7, .6, .5)), b.Lambertian(b.SolidColor(.2, .3, .8))
    world = []
    for k in range(30):
        x, z = -2. + 0.45 * (k % 10), -1. + 0.9 * (k // 10)
        world.append(b.Triangle((x, 0.02 * k, z), (x + 0.4, 0.1, z + 0.03), (x + 0.2, 0.9 + 0.01 * k, z + 0.1), grey))
    world.append(b.Quad((-1., 0.05, -0.5), (1.5, 0., 0.), (0., 1.2, 0.4), blue))
    world.append(b.Sphere((0.7, 0.5, 0.4), 0.45, b.Lambertian(b.SolidColor(.8, .3, .3))))
    world.append(b.Quad((-3., -0.2, -3.), (6., 0., 0.), (0., 0., 6.), grey))
    world.append(b.Quad((-1., 3., -1.), (2., 0., 0.), (0., 0., 2.), b.DiffuseLight(6., 6., 6.)))
    cam = CameraConfig(45., 0., (0.5, 1.5, 5.), (0., 0.4, 0.), (0., 1., 0.))
    sc = b.finish(b.Bvh(world), cam, (.2, .3, .4), RenderConfig(64, 48, 16, PathTracingShader(8)))
    img, st, _ = _render(sc, 16, counted=True)
    assert st["triangle_tests"] > 0 and st["quad_tests"] > 0 and st["sphere_tests"] > 0, st
    _assert_parity(sc, 16, img)


def test_medium_scene_keeps_depth_one_and_equals_the_oracle():
    sc = scenes.create_test_scene(RenderConfig(64, 32, 16))
    assert sc.desc.n_mediums > 0
    _assert_parity(sc, 16)


def test_needle_scene_restarts_from_an_empty_queue():
    import random_scenes
    sc = random_scenes.needle_scene(3)
    img, _, info = _render(sc, 16)
    assert info["strict_triangles"], info
    _assert_parity(sc, 16, img)


def test_query_and_radiance_after_a_render_on_the_same_handle():
    """sol_query and sol_radiance step their searches at depth 1: closest hits equal the float oracle's, and the radiance of the frame's
    camera rays is the render's frame bit for bit - one frame from kernels of both depths."""
    from test_gpu_node_visit import OUTSIDE, as_rays, directions, oracle_hits, shell_scene
    from test_gpu_radiance import assert_render_identity
    sc = shell_scene(32, 32, 1)
    d = directions()[:64]
    rays = np.concatenate([as_rays(np.zeros((len(d), 3)), d), as_rays(np.tile(OUTSIDE, (len(d), 1)), -d)])
    status, t, mat = oracle_hits(sc, rays)
    with DeviceScene(sc) as ds:
        ds.render(0, 16, pu.SEED)
        hits = ds.closest_hits(rays)
        assert (hits["status"] == status).all() and (hits["t"].view(np.uint32) == t.view(np.uint32)).all()
        for s in (0, 5):
            assert_render_identity(ds, sc, s)


def test_range_split_and_partition_change_no_bit():
    sc = scenes.sponza_like(RenderConfig(64, 64, 32), n_triangles=4000, texture_size=64)
    with DeviceScene(sc) as ds:
        ds.render(0, 32, pu.SEED)
        whole = ds.read()
        ds.clear()
        ds.render(0, 16, pu.SEED)
        ds.render(16, 16, pu.SEED)
        split = ds.read()
        parts = []
        for rank in (1, 0):
            ds.set_partition(rank, 2)
            ds.clear()
            ds.render(0, 32, pu.SEED)
            parts.append(ds.read())  # (sol_read writes 0 for the pixels of the other rank)
    assert np.isfinite(whole).all() and whole.mean() > 0
    assert (split == whole).all()
    assert (parts[0] + parts[1] == whole).all()
