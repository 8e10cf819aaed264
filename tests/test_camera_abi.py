"""Moving the camera of a live scene (sol_scene_set_camera), the part that needs no GPU: solh_camera is Camera::new on its
own - the bytes finish() puts into the description -, the two entry points are exported and refuse bad arguments with SOL_EINVAL before any
device is touched, and the proof kernel is gfx950 code of the library. Nothing new computes without a GPU."""
import ctypes as C
import os
import re

import pytest

from solstrale_amd import CameraConfig, PathTracingShader, RenderConfig, SceneBuilder, _abi, camera_record, scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "solstrale_hip.h")


def _pinhole_scene(rc):
    b = SceneBuilder()
    cam = CameraConfig(37., 0., (3., 2., 9.), (0.5, 1., 0.), (0.1, 1., 0.))
    world = [b.Sphere((0., 1., 0.), 1., b.DiffuseLight(4., 4., 4.)), b.Sphere((2., 0.5, -1.), .5, b.Lambertian(b.SolidColor(.5, .5, .5)))]
    return b.finish(b.Bvh(world), cam, (.2, .3, .5), rc), cam


@pytest.mark.parametrize("name", ["thin_lens_test_scene", "pinhole"])
def test_solh_camera_is_the_camera_field_of_finish_byte_for_byte(name):
    if name == "pinhole":
        sc, cam = _pinhole_scene(RenderConfig(123, 77, 1))
        assert cam.aperture_size == 0.
    else:
        sc = scenes.create_test_scene(RenderConfig(200, 100, 1, PathTracingShader(8)))
        cam = scenes.create_test_scene_camera()
        assert cam.aperture_size > 0.
    rec = camera_record(sc.width, sc.height, cam)
    assert isinstance(rec, _abi.SolCamera)
    assert bytes(rec) == bytes(sc.desc.camera)
    assert (rec.lens_radius > 0.) == (name != "pinhole")
    # another frame size is another camera (the aspect ratio): the record is a function of all three arguments
    assert bytes(camera_record(sc.width + 8, sc.height, cam)) != bytes(rec)


def test_solh_camera_refuses_null_pointers():
    lib = _abi.load_host()
    out = _abi.SolCamera()
    v = _abi.d3((0., 0., 1.))
    assert lib.solh_camera(16, 16, 40., 0., None, v, v, C.byref(out)) < 0
    assert lib.solh_camera(16, 16, 40., 0., v, v, v, None) < 0
    assert b"null" in lib.solh_last_error()


def test_the_entry_points_are_exported_and_the_header_states_the_contract():
    lib = _abi.load_hip()
    for name in ("sol_scene_set_camera", "sol_scene_background_flags"):
        assert hasattr(lib, name) and name in _abi.HIP_SYMBOLS
    assert hasattr(_abi.load_host(), "solh_camera") and "solh_camera" in _abi.HOST_SYMBOLS
    text = open(HEADER).read()
    assert re.search(r"#define SOL_CAMERA_NO_BACKGROUND_PROOF\s+1u", text) and _abi.SOL_CAMERA_NO_BACKGROUND_PROOF == 1
    assert re.search(r"#define SOL_CAMERA_REPROBE\s+2u", text) and _abi.SOL_CAMERA_REPROBE == 2
    assert re.search(r"typedef struct SolCameraUpdate \{ uint32_t size, flags, reserved\[2\]; \} SolCameraUpdate;", text)
    assert C.sizeof(_abi.SolCameraUpdate) == 16
    assert [(n, getattr(_abi.SolCameraUpdate, n).offset) for n, _ in _abi.SolCameraUpdate._fields_] == [("size", 0), ("flags", 4), ("reserved", 8)]


def test_the_proof_kernel_is_gfx950_code_of_the_library():
    assert b"sol_background_proof_kernel" in open(_abi.HIP_LIB, "rb").read()


def test_argument_errors_are_einval_before_the_device():
    """What can be refused without a handle: a null scene, a null camera, a null n_found - with or without a GPU. (The struct's size, flag
    bits and reserved fields need a handle behind them to be reached: tests/test_gpu_set_camera.py.)"""
    lib = _abi.load_hip()
    cam = _abi.SolCamera()
    upd = _abi.SolCameraUpdate(size=C.sizeof(_abi.SolCameraUpdate))
    assert lib.sol_scene_set_camera(None, C.byref(cam), C.byref(upd)) == _abi.SOL_EINVAL
    assert b"null scene" in lib.sol_last_error()
    assert lib.sol_scene_set_camera(None, None, None) == _abi.SOL_EINVAL
    n = C.c_uint32(7)
    flags = (C.c_uint8 * 4)()
    assert lib.sol_scene_background_flags(None, flags, 4, C.byref(n)) == _abi.SOL_EINVAL
    assert lib.sol_scene_background_flags(None, None, 0, None) == _abi.SOL_EINVAL
    assert n.value == 7
