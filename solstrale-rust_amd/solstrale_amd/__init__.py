"""solstrale_amd -- Python harness over the MI355X path-tracing library (tests/, bench.py).

The product is native: `_build/libsolstrale_hip.so` (hand-written HIP kernels for gfx950 behind the C ABI of
include/solstrale_hip.h) and `_build/libsolstrale_host.so` (C++ mirror of the reference's host surface). This package only
binds them with ctypes; it contains no rendering code and no CPU fallback.
"""
from . import _abi  # noqa: F401
from .host import (AdaptiveSampling, AlbedoShader, BloomPostProcessor, CameraConfig, DenoisePostProcessor, HostError, NopPostProcessor, NormalShader, OidnPostProcessor,  # noqa: F401
                   PathTracingShader, RenderConfig, RotationX, RotationY, RotationZ, Scale, Scene, SceneBuilder, SimpleShader,
                   Translation, camera_record)
from .device import MOMENTS_DTYPE, moments_mean_variance, moments_to_numpy  # noqa: F401
from .device import CHART_NONE, DEPTH_TEXEL_DTYPE, LIGHTMAP_TEXEL_DTYPE, OCT_TEXEL_DTYPE, VOLUME_PROBE_DTYPE, DeviceError, DeviceScene, VolumeGrid, lightmap_mesh, lightmap_mip_layout, lightmap_texels_to_numpy, lightmap_triangle_table, lightmap_unwrap, lightmap_unwrap_fit, UnwrapResult, volume_probes_to_numpy, background_blocks, comm_unique_id, device_count, pixel_spread, quad_from_corner, record_sizes, sh9, sh9_irradiance, sphere_from_center, triangle_from_vertices, world_tree_check  # noqa: F401
