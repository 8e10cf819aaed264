"""What the irradiance tests share (tests/test_irradiance_abi.py on the CPU, tests/test_gpu_irradiance.py on the device): the generator's
directions as the float oracle draws them, the orthonormal basis restated in numpy float64, and the occluder scene's prediction - which of
a point's directions a sphere on its normal blocks."""
import numpy as np

import orc

# The occluder case: a sphere of radius R centred D along the normal of a point at the origin. Seen from the point it fills the cone of
# half-angle asin(R / D) about the normal; a cosine-weighted direction falls inside with probability sin^2 = (R / D)^2, a uniform one over
# the whole sphere with (1 - cos) / 2.
OCC_RATIO = 0.6
OCC_D = 2.0
OCC_R = OCC_RATIO * OCC_D
OCC_SEED = 0x5EED0CC1
OCC_KEY_BASE = 1000
OCC_POINTS, OCC_SAMPLES = 64, 1024
OCC_NORMAL = np.array([0.3, 0.9, -0.2])  # (not unit length: the queries do not ask for it)
OCC_EDGE = 1e-4  # rad: a direction this close to the cone's edge is borderline - fp32 and float64 may disagree about it


def stream_rows(seed, keys, samples):
    """The rows the function tables take for every (key, sample): (seed low word, seed high word, key, sample) as bit patterns in float32,
    key-major."""
    keys, samples = np.asarray(keys, dtype=np.uint32), np.asarray(samples, dtype=np.uint32)
    x = np.empty((len(keys), len(samples), 4), dtype=np.uint32)
    x[..., 0], x[..., 1] = seed & 0xFFFFFFFF, seed >> 32
    x[..., 2], x[..., 3] = keys[:, None], samples[None, :]
    return x.reshape(-1, 4).view(np.float32)


def local_cosine_directions(seed, keys, samples):
    """random_cosine_direction from the stream of (seed, key, sample) at counter 0, in the float oracle (function 8 of its table):
    [len(keys), len(samples), 3] float32, in the local frame (z = the normal)."""
    y = orc.eval_f32(8, stream_rows(seed, keys, samples), 7)
    return y[:, 0:3].reshape(len(keys), len(samples), 3)


def sphere_draws_after_the_cosine(seed, keys, samples):
    """Function 8 draws random_in_unit_sphere right after the cosine direction, that is from counter 2 on: the accepted point (not
    normalised), [k, s, 3] float32, and the counter afterwards, [k, s] uint32 - 2 + 3 x rejection rounds."""
    y = orc.eval_f32(8, stream_rows(seed, keys, samples), 7)
    return y[:, 3:6].reshape(len(keys), len(samples), 3), np.ascontiguousarray(y[:, 6]).view(np.uint32).reshape(len(keys), len(samples))


def onb(normal):
    """onb_new (the reference's geo/mod.rs:245-257) in float64: (tangent, bi_tangent, unit normal)."""
    w = np.asarray(normal, dtype=np.float64)
    uw = w / np.sqrt((w * w).sum())
    a = np.array([0., 1., 0.]) if abs(uw[0]) > 0.9 else np.array([1., 0., 0.])
    v = np.cross(uw, a)
    v = v / np.sqrt((v * v).sum())
    return np.cross(uw, v), v, uw


def world_directions(normal, local):
    """onb_local in float64: tangent * x + bi_tangent * y + normal * z."""
    u, v, w = onb(normal)
    local = np.asarray(local, dtype=np.float64)
    return local[..., 0:1] * u + local[..., 1:2] * v + local[..., 2:3] * w


def cone_classes(normal, dirs, ratio=OCC_RATIO, edge=OCC_EDGE):
    """(blocked, borderline) per direction: the angle to the normal against the cone of half-angle asin(ratio)."""
    _, _, w = onb(normal)
    d = np.asarray(dirs, dtype=np.float64)
    cosang = (d * w).sum(axis=-1) / np.sqrt((d * d).sum(axis=-1))
    ang = np.arccos(np.clip(cosang, -1.0, 1.0))
    half = np.arcsin(ratio)
    return ang < half, np.abs(ang - half) < edge


def occluder_prediction():
    """The occluder case in COSINE mode at first_draw = 0: per (point, sample) whether the direction is blocked and whether it is borderline."""
    keys = OCC_KEY_BASE + np.arange(OCC_POINTS)
    local = local_cosine_directions(OCC_SEED, keys, np.arange(OCC_SAMPLES))
    return cone_classes(OCC_NORMAL, world_directions(OCC_NORMAL, local))
