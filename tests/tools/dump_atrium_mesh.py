"""Writes scenes.atrium_mesh (C3's triangles) as float32 [n][3][3] for search_schedule_sim.cpp (not a pytest, no GPU).
Usage: python tests/tools/dump_atrium_mesh.py out.bin [n_triangles] [regular|heterogeneous]"""
import _paths  # noqa: F401  (sys.path)
import sys

import numpy as np

from solstrale_amd import scenes

n = int(sys.argv[2]) if len(sys.argv) > 2 else scenes.SPONZA_TRIANGLES
tris, _, _ = scenes.atrium_mesh(n, mesh=sys.argv[3] if len(sys.argv) > 3 else "regular")
np.ascontiguousarray(tris, dtype=np.float32).tofile(sys.argv[1])
print(f"{len(tris)} triangles -> {sys.argv[1]}")
