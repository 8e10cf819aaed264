// sol_sh.h -- the real spherical-harmonic basis up to l = 2 that the SH irradiance queries project onto (include/solstrale_hip.h,
// sol_irradiance_sh). One text: sol_sh_project_kernel (sol_radiance.hip) calls it, the Python `sh9` and the tests restate it.
//
// Order (l, m) = (0,0), (1,-1), (1,0), (1,1), (2,-2), (2,-1), (2,0), (2,1), (2,2); no Condon-Shortley sign; evaluated on d = (x, y, z) as it
// comes, not normalised. Every operation is one fp32 rounding (the build's -ffp-contract=off: no fused multiply-add), in this bracketing:
//   Y0 = k0                 Y1 = k1 * y               Y2 = k1 * z
//   Y3 = k1 * x             Y4 = (k2 * x) * y         Y5 = (k2 * y) * z
//   Y6 = k3 * ((3 * (z * z)) - 1)                     Y7 = (k2 * x) * z         Y8 = k4 * ((x * x) - (y * y))
// with the constants the fp32 roundings of sqrt(1/(4 pi)), sqrt(3/(4 pi)), sqrt(15/(4 pi)), sqrt(5/(16 pi)), sqrt(15/(16 pi)).
#pragma once
#include "sol_math.h"

#define SOL_SH9_K0 0.28209479177387814f
#define SOL_SH9_K1 0.4886025119029199f
#define SOL_SH9_K2 1.0925484305920792f
#define SOL_SH9_K3 0.31539156525252005f
#define SOL_SH9_K4 0.5462742152960396f

DEV void sh9_basis(f3 d, float (&Y)[9]) {
  const float x = d.x, y = d.y, z = d.z;
  Y[0] = SOL_SH9_K0;
  Y[1] = SOL_SH9_K1 * y;
  Y[2] = SOL_SH9_K1 * z;
  Y[3] = SOL_SH9_K1 * x;
  Y[4] = (SOL_SH9_K2 * x) * y;
  Y[5] = (SOL_SH9_K2 * y) * z;
  Y[6] = SOL_SH9_K3 * ((3.0f * (z * z)) - 1.0f);
  Y[7] = (SOL_SH9_K2 * x) * z;
  Y[8] = SOL_SH9_K4 * ((x * x) - (y * y));
}
