// sol_wave.h -- the pieces of the persistent-wave schedule, shared by the kernels that are assembled from them:
// sol_render_kernel, sol_radiance_kernel, sol_query_kernel, sol_visibility_kernel and the A/B sol_render_pool4_kernel. Every piece is force-inlined; the
// __shared__ arrays stay declared in the kernels (LDS layout is per kernel) and come in as pointers.
//   wave_search_stack     the search context of a lane: LDS stack, spill tail, pinned node fields, octant and selector tables
//   wave_reservoir        the wave's reserved work items in LDS, zeroed; wave_take_item hands them out
//   wave_keeps_searching  the search loop's leave vote
// (trav_begin_world / trav_restart_world, a search from the scene's root and the same ray searched again: sol_trace.h)
#pragma once
#include <type_traits>

#include "sol_path.h"

// Fills `st` for the calling lane and the workgroup's tables; ends with the barrier behind which the tables may be read.
// lds_depth: entries per lane of `lds_stack`; may_spill = false: built for scenes whose searches fit it (every stack access is a plain LDS
// access, the spill branches and their waits fold away). sel_table may be nullptr: the node test then picks its plane words with selects.
// (Decided by the argument's type, not its value: offset 0 is a valid LDS address, so a run-time test of a __shared__ array's address
// does not fold, and a kernel would carry both node tests - 1.4 KiB more code and other registers in every instance.)
template <class SelTable>
DEV void wave_search_stack(Stack& st, const DevScene& S, uint32_t* lds_stack, int lds_depth, bool may_spill, uint32_t* spill, uint32_t total_threads,
                           uint8_t* oct_table, SelTable sel_table) {
  const uint32_t tid = threadIdx.x;
  st.lds = (lds_u32*)lds_stack + tid;
  st.spill = (SOL_AS1 uint32_t*)spill + (blockIdx.x * SOL_WG + tid);
  st.stride = total_threads;
  st.depth = may_spill ? lds_depth : SOL_NO_SPILL;
  sol_search_context<true>(st, S);
  sol_fill_oct_table((lds_u8*)oct_table, tid, SOL_WG);
  st.oct_table = (const lds_u8*)oct_table;
  st.oct_table_on = true;
  if constexpr (SOL_SEL_TABLE && !std::is_null_pointer<SelTable>::value) {
    sol_fill_sel_table((lds_u32*)sel_table, tid, SOL_WG);
    st.sel_table = (const lds_u32*)sel_table;
    st.sel_table_on = true;
  }
  __syncthreads();
}

// The calling wave's reservoir out of the workgroup's, emptied by the wave's first lane: [0] the next reserved item, [1] the end of the
// reservation. The only way to what wave_take_item takes, so no kernel starts with an uninitialised one. Only its own wave touches it,
// and one wave's LDS operations execute in order: no barrier. volatile: the leader's stores and every lane's loads must stay real LDS
// accesses in program order (without it the compiler may forward a stale value to the non-leader lanes).
DEV volatile lds_u32* wave_reservoir(uint32_t (&reservoirs)[SOL_WG / 64][2]) {
  uint32_t* res = reservoirs[threadIdx.x >> 6];
  if ((threadIdx.x & 63u) == 0u) { res[0] = 0u; res[1] = 0u; }
  return (volatile lds_u32*)res;
}

// The next item of the work order for every lane that calls (the callers are the wave's lanes without one). The wave refills its
// reservoir 64 items at a time - an aligned run of the work order: one 8x8 pixel block of one chunk, 64 consecutive rays - with ONE
// returning atomic; lanes take consecutive items from it by popcount prefix. The wave thus waits for the global counter (1-3 us under
// load, ~88 dequeues/us per address) once per 64 items instead of once per service pass.
DEV uint32_t wave_take_item(volatile lds_u32* res, uint32_t* __restrict__ work_counter, uint32_t lane) {
  const unsigned long long need = sol_ballot(true);
  const uint32_t leader = (uint32_t)__ffsll((long long)need) - 1u;
  const uint32_t n_need = (uint32_t)__popcll(need), my = (uint32_t)__popcll(need & ((1ull << lane) - 1ull));
  const uint32_t next = res[0], left = res[1] - next;
  uint32_t fresh = 0;
  if (n_need > left) {  // take what is left, then continue in a fresh block of 64
    if (lane == leader) fresh = atomicAdd(work_counter, 64u);
    fresh = __shfl(fresh, (int)leader);
  }
  if (lane == leader) {
    res[0] = n_need > left ? fresh + (n_need - left) : next + n_need;
    if (n_need > left) res[1] = fresh + 64u;
  }
  return my < left ? next + my : fresh + (my - left);
}

// The search loop's vote, once per step: does the wave take another step? It leaves for the service block when none of its lanes is
// searching (`act`), or when too few are while others wait: fewer than switch_below 64ths of the live lanes (0: only when none is).
DEV bool wave_keeps_searching(bool act, uint32_t switch_below) {
  const unsigned long long am = sol_ballot(act);
  if (am == 0ull) return false;
  const unsigned long long live = sol_ballot(true);
  return am == live || (uint32_t)__popcll(am) * 64u >= switch_below * (uint32_t)__popcll(live);
}
