"""sol_scene_set_camera: a live handle looks at its scene through another camera. After the move every output is byte-identical
to a handle freshly created with that camera; the background blocks are proved again by sol_background_proof_kernel over the device tree and
equal the host proof's over the same tree; a flagged block's camera rays all miss on the device itself; what creation would not prove is not
proved; sums and sessions are reset, options, modes and the partition kept; a camera path through one handle allocates nothing more.

Frames are at most 128x96 and renders 16 samples. The camera pairs are first checked on the CPU (background_blocks): each camera flags at
least a tenth of the blocks and the two sets differ in at least a tenth - a handle that kept the old table, or adopted none, would be caught."""
import ctypes as C
import math

import numpy as np
import pytest

import parity_util as pu
from solstrale_amd import (CameraConfig, DeviceError, DeviceScene, PathTracingShader, RenderConfig, SceneBuilder, _abi, background_blocks,
                           camera_record, scenes)

pytestmark = pytest.mark.gpu

SEED = pu.SEED
SPP = 16
RC = RenderConfig(128, 96, SPP, PathTracingShader(8))


def _statue():  # pinhole, open sky, a triangle mesh: the device build pre-splits and reinserts
    return scenes.statue_like(RC, n_triangles=20000)


def _lens_balls(rc=RC):  # a thin lens and no constant medium (ray queries refuse a scene with one)
    b = SceneBuilder()
    grey = b.Lambertian(b.SolidColor(.6, .6, .6))
    world = [b.Sphere((-1.5, 1., 0.), .6, b.DiffuseLight(6., 6., 6.)), b.Sphere((1.2, 1.3, -2.), .5, grey),
             b.Triangle((-.5, 0., 1.), (.5, 0., 1.), (0., .9, 1.), grey), b.Quad((-3., 0., -3.), (6., 0., 0.), (0., 0., 6.), grey)]
    return b.finish(b.Bvh(world), _PAIRS["lens_balls"][0], (.2, .3, .5), rc)


# scene -> (maker, camera A, camera B); None: the proof does not apply (a closed box, an environment map)
_PAIRS = {
    "statue": (CameraConfig(38., 0., (4.5, 3.6, 8.0), (0.2, 2.6, 0.), (0., 1., 0.)), CameraConfig(50., 0., (0., 9., 9.), (0.2, 2.6, 0.), (0., 1., 0.))),
    "test_scene": (CameraConfig(40., 0.1, (-5., 3., 6.), (-3., 4., -6.), (0., 1., 0.)), CameraConfig(50., 0.1, (-8., 2., -4.), (0., 3., -2.), (0., 1., 0.))),
    "lens_balls": (CameraConfig(35., 0.3, (0., 2.5, 8.), (0., 1.5, 0.), (0., 1., 0.)), CameraConfig(45., 0.2, (7., 2., 4.), (0., 1.5, 0.), (0., 1., 0.))),
    "cornell": (CameraConfig(**scenes._CORNELL_CAMERA), CameraConfig(30., 0., (200., 300., -700.), (278., 200., 0.), (0., 1., 0.))),
    "environment": (scenes.create_test_scene_camera(), CameraConfig(40., 0.1, (-5., 3., 6.), (-3., 4., -6.), (0., 1., 0.))),
}
_MAKERS = {"statue": _statue, "test_scene": lambda: scenes.create_test_scene(RC), "lens_balls": _lens_balls,
           "cornell": lambda: scenes.cornell_box(RC), "environment": lambda: scenes.create_test_scene_with_environment(RC)}
_PROVED = ("statue", "test_scene", "lens_balls")
_scene_cache = {}

# A frame of 100x52: 13x7 = 91 blocks - two workgroups of the proof kernel, the second partly empty - with edge blocks in x and in y.
RAGGED = RenderConfig(100, 52, SPP, PathTracingShader(8))
_RAGGED = {"ragged_lens_balls": "lens_balls", "ragged_statue": "statue"}
_MAKERS["ragged_lens_balls"] = lambda: _lens_balls(RAGGED)
_MAKERS["ragged_statue"] = lambda: scenes.statue_like(RAGGED, n_triangles=20000)
for _ragged, _plain in _RAGGED.items():
    _PAIRS[_ragged] = _PAIRS[_plain]

CHAIN_LEVELS = 48
_PAIRS["chain"] = (CameraConfig(40., 0., (0., 1., 16.), (0., 0., 0.), (0., 1., 0.)), CameraConfig(40., 0.2, (9., 4., 11.), (0., 0., 0.), (0., 1., 0.)))


def _chain():
    """Spheres along a line whose caller-given BVH is a chain: every node holds one sphere and the rest, CHAIN_LEVELS levels deep."""
    b = SceneBuilder()
    grey = b.Lambertian(b.SolidColor(.6, .6, .6))
    balls = [b.Sphere((-6. + 12. * k / CHAIN_LEVELS, .3 * math.sin(k), .3 * math.cos(2. * k)), .22, b.DiffuseLight(4., 4., 4.) if k == 0 else grey) for k in range(CHAIN_LEVELS + 1)]
    rest = balls[-1]
    for ball in reversed(balls[:-1]):
        rest = b.Bvh([ball, rest])
    return b.finish(rest, _PAIRS["chain"][0], (.2, .3, .5), RC)


_MAKERS["chain"] = _chain


def _scene(name, cam):
    """The scene `name` with `cam` in its description (the description's camera field is Camera::new of it: tests/test_camera_abi.py)."""
    if name not in _scene_cache:
        _scene_cache[name] = _MAKERS[name]()
    sc = _scene_cache[name]
    sc.desc.camera = camera_record(sc.width, sc.height, cam)
    return sc


def _pixel_mask(flags, sc):
    return np.repeat(np.repeat(flags, 8, axis=0), 8, axis=1)[:sc.height, :sc.width]


@pytest.fixture(scope="module", autouse=True)
def the_camera_pairs_exercise_the_proof():
    """On the CPU: both cameras of a pair flag at least a tenth of the blocks, and the flag sets differ in at least a tenth of them."""
    for name in _PROVED:
        a, b = _PAIRS[name]
        fa, fb = background_blocks(_scene(name, a), 0).copy(), background_blocks(_scene(name, b), 0).copy()
        assert fa.mean() >= 0.1 and fb.mean() >= 0.1 and (fa != fb).mean() >= 0.1, (name, fa.mean(), fb.mean(), (fa != fb).mean())
    for name in _RAGGED:  # the 16-bin host tree the ragged case is created with: both cameras flag something at that size
        for cam in _PAIRS[name]:
            f = background_blocks(_scene(name, cam), 1)
            assert f.shape == (7, 13) and f.any(), name
    for cam in _PAIRS["chain"]:  # the reference's topology: neither everything nor nothing is flagged
        f = background_blocks(_scene("chain", cam), 0)
        assert 0.1 <= f.mean() <= 0.9, f.mean()


def _outputs(ds, aux=True):
    ds.render(0, SPP, SEED)
    out = [ds.read()]
    if aux:
        ds.render_aux(0, SPP, SEED)
        out += list(ds.read_aux())
    out.append(ds.camera_rays(0, 0, ds.width, ds.height, 3, SEED).cpu().numpy())
    return out


def _same(got, want, what):
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes(), (what, k, int((g != w).sum()))


_VARIANTS = {
    "default": dict(),
    "sah16": dict(world_tree=_abi.TREE_SAH16),
    "blocks_option_0": dict(option=(_abi.OPT_BACKGROUND_BLOCKS, 0)),
    "no_proof": dict(move=dict(background_proof=False)),
    "reprobe": dict(move=dict(reprobe=True)),
}


@pytest.mark.parametrize("variant", list(_VARIANTS))
@pytest.mark.parametrize("name", ["statue", "test_scene", "cornell", "environment"])
def test_a_moved_handle_renders_what_a_fresh_handle_renders(name, variant):
    """1. Created with camera A, rendered (the table, the costs and the sums are A's), moved to B: frame, auxiliary planes and camera rays are
    those of a fresh handle of the same scene with camera B - byte for byte."""
    v = _VARIANTS[variant]
    cam_a, cam_b = _PAIRS[name]
    create = dict(world_tree=v.get("world_tree"))

    def configured(sc):
        ds = DeviceScene(sc, **create)
        if "option" in v:
            ds.set_option(*v["option"])
        return ds

    with configured(_scene(name, cam_b)) as fresh:
        want = _outputs(fresh)
        want_flags = fresh.background_flags()
    with configured(_scene(name, cam_a)) as ds:
        stale = _outputs(ds)
        assert stale[0].tobytes() != want[0].tobytes()
        ds.set_camera(cam_b, **v.get("move", {}))
        _same(_outputs(ds), want, (name, variant))
        if variant == "no_proof":
            assert not ds.background_flags().any() and ds.info()["background_blocks"] == 0
        elif variant == "sah16":  # a host-built tree is the same tree on both sides: the host proof of the fresh handle flags the same blocks
            assert (ds.background_flags() == want_flags).all()
        if name in _PROVED and variant != "no_proof":
            assert ds.background_flags().mean() >= 0.1


@pytest.mark.parametrize("tree", [None, _abi.TREE_SAH16])
@pytest.mark.parametrize("name", ["statue", "test_scene", "lens_balls"])
def test_the_device_proof_flags_what_the_host_proof_flags(name, tree):
    """2. Creation's flags are the host proof over the handle's tree: moving to the creation camera proves the same tree on the device and
    must flag the same blocks. With the 16-bin host tree the diagnostic builds the same tree, so camera B's flags are known too."""
    cam_a, cam_b = _PAIRS[name]
    with DeviceScene(_scene(name, cam_a), world_tree=tree) as ds:
        created = ds.background_flags()
        assert created.mean() >= 0.1
        ds.set_camera(cam_a)
        assert (ds.background_flags() == created).all(), int((ds.background_flags() != created).sum())
        ds.set_camera(cam_b)
        moved = ds.background_flags()
        sc_b = _scene(name, cam_b)
        if tree == _abi.TREE_SAH16:
            assert (moved == background_blocks(sc_b, 1)).all()
        info = ds.info()
        assert info["background_blocks"] == int(moved.sum()) and info["background_pixels"] == int(_pixel_mask(moved, sc_b).sum())
        ds.set_camera(cam_a)  # and back
        assert (ds.background_flags() == created).all()


@pytest.mark.parametrize("name", list(_RAGGED))
def test_the_device_proof_on_a_ragged_frame(name):
    """2a. 91 blocks in two workgroups, the last lanes of the second without a block, edge blocks of 4 pixels in x and in y: with the 16-bin
    host tree the flags after each move are the host proof's over the same tree."""
    cam_a, cam_b = _PAIRS[name]
    with DeviceScene(_scene(name, cam_a), world_tree=_abi.TREE_SAH16) as ds:
        for cam in (cam_a, cam_b, cam_a):
            ds.set_camera(cam)
            want = background_blocks(_scene(name, cam), 1)
            assert (ds.background_flags() == want).all(), (name, int((ds.background_flags() != want).sum()))
            assert ds.info()["background_blocks"] == int(want.sum()) and ds.info()["background_pixels"] == int(_pixel_mask(want, _scene(name, cam)).sum())


def test_the_device_proof_on_a_deep_tree():
    """2b. A chain of CHAIN_LEVELS binary nodes, created with the host tree that keeps the reference's topology: the walk goes down level after
    level through its one stack entry per level, and flags what the host proof (the diagnostic, over the same tree) flags."""
    cam_a, cam_b = _PAIRS["chain"]
    with DeviceScene(_scene("chain", cam_a), world_tree=_abi.TREE_REF) as ds:
        assert (ds.background_flags() == background_blocks(_scene("chain", cam_a), 0)).all()
        for cam in (cam_b, cam_a):
            ds.set_camera(cam)
            want = background_blocks(_scene("chain", cam), 0)
            assert (ds.background_flags() == want).all(), int((ds.background_flags() != want).sum())


@pytest.mark.parametrize("name", ["statue", "lens_balls"])
def test_every_camera_ray_of_a_flagged_block_misses_on_the_device(name):
    """3. Soundness without the host: the rays the render would start in the flagged blocks (samples 0..3, the test's seed) hit nothing."""
    cam_a, cam_b = _PAIRS[name]
    sc = _scene(name, cam_a)
    with DeviceScene(sc) as ds:
        ds.set_camera(cam_b)
        mask = _pixel_mask(ds.background_flags(), sc)
        assert mask.mean() >= 0.1
        hits_elsewhere = 0
        for sample in range(4):
            rays = ds.camera_rays(0, 0, sc.width, sc.height, sample, SEED)
            status = ds.occluded(rays.reshape(-1, 8)).cpu().numpy().reshape(sc.height, sc.width)
            assert (status[mask] == _abi.SOL_RAY_MISS).all(), (name, sample, int((status[mask] != _abi.SOL_RAY_MISS).sum()))
            hits_elsewhere += int((status[~mask] == _abi.SOL_RAY_HIT).sum())
        assert hits_elsewhere > 0


def _far_scene(offset, rc):  # (tests/test_background_blocks.py, test_a_camera_far_from_the_origin_widens_the_margin_or_gives_up)
    b = SceneBuilder()
    cam = CameraConfig(2., 0., (offset, 0., 500.), (offset, 0., 0.), (0., 1., 0.))
    world = [b.Sphere((offset, 0., 0.), 3., b.DiffuseLight(5., 5., 5.)), b.Sphere((offset + 2., 1., -20.), 2.5, b.Lambertian(b.SolidColor(.5, .5, .5)))]
    return b.finish(b.Bvh(world), cam, (.2, .3, .5), rc), cam


def test_no_flags_where_the_proof_does_not_apply():
    """4. An environment map, a handle created without background blocks, a camera whose fp32 rays err by more than three pixels,
    background_proof=False."""
    cam_a, cam_b = _PAIRS["environment"]
    with DeviceScene(_scene("environment", cam_a)) as ds:
        ds.set_camera(cam_b)
        assert not ds.background_flags().any() and ds.info()["background_blocks"] == 0
    cam_a, cam_b = _PAIRS["statue"]
    with DeviceScene(_scene("statue", cam_a), no_background_blocks=True) as ds:
        assert not ds.background_flags().any()
        ds.set_camera(cam_b)
        assert not ds.background_flags().any() and ds.info()["background_pixels"] == 0
    with DeviceScene(_scene("statue", cam_a)) as ds:
        assert ds.background_flags().any()
        ds.set_camera(cam_b, background_proof=False)
        assert not ds.background_flags().any()
        ds.set_camera(cam_b)
        assert ds.background_flags().any()
    near, near_cam = _far_scene(1e4, RenderConfig(128, 96, SPP))
    with DeviceScene(near) as ds:
        assert ds.background_flags().any()
        ds.set_camera(CameraConfig(2., 0., (2e6, 0., 500.), (2e6, 0., 0.), (0., 1., 0.)))
        assert not ds.background_flags().any()
        ds.set_camera(near_cam)
        assert ds.background_flags().any()


def test_sums_and_sessions_are_reset():
    """5a. The accumulator and the auxiliary planes read zero after a move; an adaptive session is over, as after sol_clear."""
    cam_a, cam_b = _PAIRS["statue"]
    with DeviceScene(_scene("statue", cam_a)) as ds:
        ds.render(0, SPP, SEED)
        ds.render_aux(0, SPP, SEED)
        assert ds.read().any() and ds.read_aux()[0].any()
        ds.set_camera(cam_b)
        assert not ds.read().any()
        albedo, normal = ds.read_aux()
        assert not albedo.any() and not normal.any()
        assert ds.resolve_aux()[2] == 0
        ds.adaptive_begin(16, 16, 32, 0.05)
        assert ds.adaptive_round(SEED) > 0
        ds.set_camera(cam_a)
        with pytest.raises(DeviceError) as e:
            ds.adaptive_round(SEED)
        assert e.value.code == _abi.SOL_EINVAL and "no adaptive session" in e.value.msg
        ds.clear()
        with pytest.raises(DeviceError) as e2:
            ds.adaptive_round(SEED)
        assert e2.value.msg == e.value.msg


def test_adaptive_rounds_after_a_move_are_the_fresh_handles():
    cam_a, cam_b = _PAIRS["statue"]

    def rounds(ds):
        ds.adaptive_begin(16, 16, 32, 0.05)
        n = ds.adaptive_run(SEED)
        return n, ds.read(), ds.adaptive_counts()

    with DeviceScene(_scene("statue", cam_b)) as fresh:
        want = rounds(fresh)
    with DeviceScene(_scene("statue", cam_a)) as ds:
        ds.render(0, SPP, SEED)
        ds.set_camera(cam_b)
        got = rounds(ds)
    assert got[0] == want[0] and got[1].tobytes() == want[1].tobytes() and (got[2] == want[2]).all()


def test_the_light_sampling_mode_survives_a_move():
    """5b. sol_light_sampling("tree") set before the move still holds after it (many lights: the LT kernels run)."""
    def many(cam):
        key = "many_lights"
        if key not in _scene_cache:
            _scene_cache[key] = scenes.many_lights(64, "quads", RenderConfig(96, 96, SPP, PathTracingShader(6)))
        sc = _scene_cache[key]
        sc.desc.camera = camera_record(sc.width, sc.height, cam)
        return sc

    cam_a, cam_b = _PAIRS["cornell"]
    with DeviceScene(many(cam_b)) as fresh:
        fresh.light_sampling("tree")
        fresh.render(0, SPP, SEED)
        want = fresh.read()
    with DeviceScene(many(cam_a)) as ds:
        ds.light_sampling("tree")
        ds.render(0, SPP, SEED)
        ds.set_camera(cam_b)
        nodes_before = ds.light_tree()[0]
        ds.render(0, SPP, SEED)
        assert ds.read().tobytes() == want.tobytes()
        assert (ds.light_tree()[0] == nodes_before).all()


def test_the_partition_survives_a_move():
    """5c. Rank 1 of 2 before the move is rank 1 of 2 after it; the cost probe cannot run on a part of the frame."""
    cam_a, cam_b = _PAIRS["statue"]
    with DeviceScene(_scene("statue", cam_b)) as fresh:
        fresh.set_partition(1, 2)
        fresh.render(0, SPP, SEED)
        want, want_floats, want_crc = fresh.read(), fresh.accum_floats(), fresh.info()["partition_crc"]
    with DeviceScene(_scene("statue", cam_a)) as ds:
        ds.set_partition(1, 2)
        ds.render(0, SPP, SEED)
        frame_a = ds.read()
        with pytest.raises(DeviceError) as e:
            ds.set_camera(cam_b, reprobe=True)
        assert e.value.code == _abi.SOL_EINVAL and "world" in e.value.msg
        ds.clear()
        ds.render(0, SPP, SEED)
        assert ds.read().tobytes() == frame_a.tobytes()  # refused before anything was touched: still camera A's frame
        crc = ds.info()["partition_crc"]
        ds.set_camera(cam_b)
        ds.render(0, SPP, SEED)
        assert ds.accum_floats() == want_floats and ds.info()["partition_crc"] == want_crc == crc
        assert ds.read().tobytes() == want.tobytes()


def test_argument_errors_with_a_handle():
    """SOL_EINVAL for a null camera, a size no version of the struct had, unknown flag bits and non-zero reserved fields; the handle is untouched."""
    cam_a, cam_b = _PAIRS["lens_balls"]
    sc = _scene("lens_balls", cam_a)
    rec = camera_record(sc.width, sc.height, cam_b)
    with DeviceScene(sc) as ds:
        ds.render(0, SPP, SEED)
        before, flags = ds.read(), ds.background_flags()
        lib = ds.lib
        good = C.sizeof(_abi.SolCameraUpdate)
        assert lib.sol_scene_set_camera(ds.h, None, None) == _abi.SOL_EINVAL
        for upd in (_abi.SolCameraUpdate(size=4), _abi.SolCameraUpdate(size=4097), _abi.SolCameraUpdate(size=good, flags=4),
                    _abi.SolCameraUpdate(size=good, flags=0x80000001), _abi.SolCameraUpdate(size=good, reserved=(C.c_uint32 * 2)(0, 1)),
                    _abi.SolCameraUpdate(size=good, reserved=(C.c_uint32 * 2)(1, 0))):
            assert lib.sol_scene_set_camera(ds.h, C.byref(rec), C.byref(upd)) == _abi.SOL_EINVAL, (upd.size, upd.flags)
        n = C.c_uint32()
        short = (C.c_uint8 * 4)()
        assert lib.sol_scene_background_flags(ds.h, short, 4, C.byref(n)) == _abi.SOL_EINVAL
        assert lib.sol_scene_background_flags(ds.h, None, 0, None) == _abi.SOL_EINVAL
        assert lib.sol_scene_background_flags(ds.h, None, 0, C.byref(n)) == _abi.SOL_OK and n.value == int(flags.sum())
        assert ds.read().tobytes() == before.tobytes() and (ds.background_flags() == flags).all()
        # a size of 8 is a struct that ends after `flags`; NULL is all zero
        assert lib.sol_scene_set_camera(ds.h, C.byref(rec), C.byref(_abi.SolCameraUpdate(size=8, flags=_abi.SOL_CAMERA_NO_BACKGROUND_PROOF))) == _abi.SOL_OK
        assert not ds.background_flags().any()
        assert lib.sol_scene_set_camera(ds.h, C.byref(rec), None) == _abi.SOL_OK
        assert ds.background_flags().any()


def test_a_camera_path_through_one_handle():
    """6. Eight cameras on an orbit at 64x48, each frame the fresh handle's; the handle allocates nothing after the second move."""
    import torch
    rc = RenderConfig(64, 48, SPP, PathTracingShader(8))
    sc = _lens_balls(rc)
    cams = [CameraConfig(40., 0.3, (8. * math.cos(2 * math.pi * k / 8), 2. + .25 * k, 8. * math.sin(2 * math.pi * k / 8)), (0., 1., 0.), (0., 1., 0.)) for k in range(8)]
    want = []
    for cam in cams:
        sc.desc.camera = camera_record(sc.width, sc.height, cam)
        with DeviceScene(sc) as fresh:
            fresh.render(0, SPP, SEED)
            want.append((fresh.read(), int(fresh.background_flags().sum())))
    assert len({w[0].tobytes() for w in want}) == 8 and any(w[1] for w in want)
    sc.desc.camera = camera_record(sc.width, sc.height, _PAIRS["lens_balls"][0])
    with DeviceScene(sc) as ds:
        ds.render(0, SPP, SEED)
        free_before = None
        for k, cam in enumerate(cams):
            if k == 2:
                torch.cuda.synchronize()
                free_before = torch.cuda.mem_get_info(ds.device)[0]
            ds.set_camera(cam)
            ds.render(0, SPP, SEED)
            assert ds.read().tobytes() == want[k][0].tobytes(), k
            assert int(ds.background_flags().sum()) == want[k][1], k
        free_after = torch.cuda.mem_get_info(ds.device)[0]
        assert free_after >= free_before, (free_before, free_after)
