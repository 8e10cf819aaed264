// sol_wide.h -- the field codec of DWide (sol_types.h has the layout), written ONCE for the host and the device: the masks, the leaf kind and
// the per-axis grid step in `meta`, a slot's plane bytes, the two 24-bit base indices in the slot-7 bytes and the implicit child addresses;
// pack_meta and set_bases on the writing side. Its readers are WideView (sol_tree.h: the host's layout, sol_world_tree_check), the
// background-block proof (sol_proof.h) and the refit (sol_geometry.hip); its writers WideLayout, k_emit (sol_build.hip) and the refit. The
// render kernel's own decode (sol_trace.h) is the one other reader of these bits: it is shaped for v_perm_b32 and stays by itself.
// `q` is a node's twelve plane words (DWide::q, or registers holding them).
#pragma once
#include <stdint.h>

#include "sol_types.h"

SOL_HD inline uint32_t sol_wide_imask(uint32_t meta) { return (meta >> 15) & 0x7Fu; }
SOL_HD inline uint32_t sol_wide_lmask(uint32_t meta) { return (meta >> 22) & 0x7Fu; }
SOL_HD inline uint32_t sol_wide_leaf_kind(uint32_t meta) { return (meta >> 29) & 3u; }
// the grid step of axis a: 2^(exponent field + emin - 127)
SOL_HD inline float sol_wide_scale(uint32_t meta, int a, uint32_t emin) { return __builtin_bit_cast(float, (((meta >> (5 * a)) & 31u) + emin) << 23); }
SOL_HD inline float sol_wide_decode(float origin, uint32_t q, float scale) { return origin + (float)q * scale; }  // == the render kernel's decode
SOL_HD inline uint32_t sol_wide_lo_byte(const uint32_t q[12], int a, int s) { return (q[2 * a + (s >> 2)] >> (8 * (s & 3))) & 0xFFu; }
SOL_HD inline uint32_t sol_wide_hi_byte(const uint32_t q[12], int a, int s) { return (q[6 + 2 * a + (s >> 2)] >> (8 * (s & 3))) & 0xFFu; }
SOL_HD inline uint32_t sol_wide_base_inner(const uint32_t q[12]) { return (q[1] >> 24) | ((q[3] >> 24) << 8) | ((q[5] >> 24) << 16); }
SOL_HD inline uint32_t sol_wide_base_prim(const uint32_t q[12]) { return (q[7] >> 24) | ((q[9] >> 24) << 8) | ((q[11] >> 24) << 16); }
// which of a mask's children slot s holds: the inner child of slot s is node base_inner + rank(imask, s), its primitive base_prim + rank(lmask, s)
SOL_HD inline uint32_t sol_wide_rank(uint32_t mask, int s) { return (uint32_t)__builtin_popcount(mask & ((1u << s) - 1u)); }

// the writing side: exponents relative to emin, masks, leaf kind; the base indices in the slot-7 bytes (top byte of each plane array's second word)
SOL_HD inline uint32_t sol_wide_pack_grid(const uint32_t e[3], uint32_t emin) { return (e[0] - emin) | ((e[1] - emin) << 5) | ((e[2] - emin) << 10); }
SOL_HD inline uint32_t sol_wide_pack_meta(const uint32_t e[3], uint32_t emin, uint32_t imask, uint32_t lmask, uint32_t leaf_kind) {
  return sol_wide_pack_grid(e, emin) | (imask << 15) | (lmask << 22) | (leaf_kind << 29);
}
SOL_HD inline uint32_t sol_wide_regrid_meta(uint32_t meta, const uint32_t e[3], uint32_t emin) { return (meta & 0xFFFF8000u) | sol_wide_pack_grid(e, emin); }  // (topology kept)
SOL_HD inline void sol_wide_set_bases(uint32_t q[12], uint32_t inner, uint32_t prim) {
  for (int k = 0; k < 3; ++k) {
    q[2 * k + 1] = (q[2 * k + 1] & 0x00FFFFFFu) | (((inner >> (8 * k)) & 0xFFu) << 24);
    q[6 + 2 * k + 1] = (q[6 + 2 * k + 1] & 0x00FFFFFFu) | (((prim >> (8 * k)) & 0xFFu) << 24);
  }
}
