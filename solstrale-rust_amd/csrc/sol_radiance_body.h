// sol_radiance_body.h -- the body of sol_radiance_kernel and of sol_radiance_each_kernel (sol_radiance.hip), included inside each: one text for
// both. It is text, not a function: a force-inlined function is optimised on its own before it is inlined, and the twenty instances of
// sol_radiance_kernel then come out with other registers and instructions than they have as plain kernels (no include guard:
// it is included twice). In scope where it is included: the kernel's arguments (Sp, P, rays, keys,
// out, partial, work_counter, spill) and the compile-time switches SPILL, STRICT, ENV, LT, GATHER, EACH.
//   EACH (with GATHER; SH irradiance queries): a work item is (point, sample), sample-major - an aligned run of 64 items is 64
//   consecutive points of one sample. The lane keeps no chunk sum and no end of a sample range, and writes the sample's 0 + colour once, one
//   dwordx4, to partial[sample - P.first_sample][point]; `out` and P.direct are not used. Everything else is as it stands.
  const DevScene& S = *Sp;
  __shared__ uint32_t lds_stack[SOL_LDS_STACK * SOL_WG];
  __shared__ uint8_t oct_table[SOL_OCT_TABLE_BYTES];
  __shared__ __attribute__((aligned(16))) uint32_t sel_table[SOL_SEL_TABLE_DWORDS];
  __shared__ uint32_t reservoir[SOL_WG / 64][2];  // per wave: next reserved item, end of the reservation
  const uint32_t lane = threadIdx.x & 63u;
  Stack st;
  wave_search_stack(st, S, lds_stack, SOL_LDS_STACK, SPILL, spill, P.total_threads, oct_table, sel_table);
  volatile lds_u32* const res = wave_reservoir(reservoir);
  Counters cnt = {};
  const float inf = __builtin_huge_valf();

  bool have_item = false, alive = false, in_flight = false;
  uint32_t index = 0, s = 0, s_end = 0;  // the item: ray `index` of the launch, samples [s, s_end) of it still to come
  f3 sum = mk3(0.f, 0.f, 0.f);
  Path p = {};
  Trav t;
  t.cur = REF_DONE;

  for (;;) {
    // ---- lanes whose search is over: the service block of sol_render_kernel, with the caller's ray and its interval at depth 0 ----
    const bool again = t.cur == REF_DONE && in_flight && sol_self_hit(p.from, t.h);  // (rule 8; a caller's ray leaves no primitive: depth > 0 only)
    // (STRICT) a refused needle hit: the lane searches the same ray again behind it - at depth 0 up to the ray's own upper end, as query_settle does
    if (STRICT && !again && t.cur == REF_DONE && in_flight && !trav_accept_or_restart(S, t, st) && p.depth == 0u) t.h.t = radiance_tmax(rays, index);
    if (t.cur == REF_DONE) {
      float tmin = RAY_MIN_F, tmax = inf;
      float4 ra = make_float4(0.f, 0.f, 0.f, 0.f), rb = ra;  // the item's ray as the work fetch of this pass loaded it
      bool fresh_ray = false;
      if (again) {
        p.o = t.o; p.d = t.d;
        tmin = sol_behind(t.h.t);
        if (p.depth == 0u) tmax = radiance_tmax(rays, index);
      } else if (in_flight) {
        in_flight = false;
        p.o = t.o; p.d = t.d;  // (the ray lives in the search state while it is traced)
        f3 c;
        if (shade_vertex<false, STRICT, ENV, LT>(S, p, t.h, c, cnt)) {
          if (!EACH) sum = sum + c;  // sums, not means: the render's chunk sum, 0 + c0 + c1 + .. in sample order
          alive = false;
          if (EACH) {
            // the item is this one sample: its colour as a query of one sample answers it (0 + c), at [sample][point] for sol_sh_project_kernel
            radiance_store(partial + (size_t)(s - P.first_sample) * (P.n_groups * 64u) + index, mk3(0.f, 0.f, 0.f) + c, 0u);
            have_item = false;
          }
          s++;
          if (!EACH && s == s_end) {
            // one chunk in the whole call: the answer itself; else the chunk sum at [chunk][ray] for sol_radiance_resolve_kernel
            if (P.direct) radiance_store(out + index, sum, P.end_sample - P.first_sample);
            else radiance_store(partial + (size_t)((s - 1u - P.first_sample) / SOL_CHUNK) * (P.n_groups * 64u) + index, sum, 0u);
            have_item = false;
          }
        }
      }
      // work fetch: the next item from the wave's reservoir (sol_wave.h) - 64 items, 64 consecutive rays of one chunk, per refill
      if (!again && !have_item) {
        const uint32_t item = wave_take_item(res, work_counter, lane);
        if (item >= P.n_items) break;  // no work left for this lane
        // item -> (ray, chunk), chunk-major: an aligned run of 64 items is 64 consecutive rays of one chunk
        // (EACH: `chunk` counts samples - (point, sample), sample-major: 64 consecutive points of one sample)
        const uint32_t pair = item >> 6, chunk = pair / P.n_groups;
        index = (pair - chunk * P.n_groups) * 64u + (item & 63u);
        if (index >= P.n_rays) continue;  // padding of the last group
        // validity, before any search (sol_ray.h): an invalid ray answers (0, 0, 0, samples = 0) - here when the kernel writes the
        // answers itself, else in the resolve kernel
        ra = ldg_f4(rays + (size_t)index * 2u); rb = ldg_f4(rays + (size_t)index * 2u + 1u);
        fresh_ray = true;  // (the first sample of the item starts from these values; the later ones read the ray again)
        if (!query_ray_valid(ra, rb)) {
          if (!EACH && P.direct) radiance_store(out + index, mk3(0.f, 0.f, 0.f), 0u);  // (EACH: sol_sh_project_kernel judges the row and reads no colour of it)
          continue;
        }
        s = P.first_sample + (EACH ? chunk : chunk * SOL_CHUNK);
        s_end = P.end_sample - s > (uint32_t)SOL_CHUNK ? s + SOL_CHUNK : P.end_sample;
        sum = mk3(0.f, 0.f, 0.f);
        have_item = true;
        alive = false;
      }
      if (!again && !alive) {
        // the path as generate_path leaves it, with the caller's ray: the RNG keyed by (seed, key, sample), its counter at first_draw
        if (!fresh_ray) { ra = ldg_f4(rays + (size_t)index * 2u); rb = ldg_f4(rays + (size_t)index * 2u + 1u); }
        const float4 a = ra, b = rb;
        uint32_t key = P.key_base + index, ctr = P.first_draw;
        if (keys) {
          const unsigned long long kw = *(const SOL_AS1 unsigned long long*)(keys + index);  // one dwordx2: pixel, first_draw
          key = (uint32_t)kw; ctr = (uint32_t)(kw >> 32);
        }
        rng_init(p.rng, P.seed_lo, P.seed_hi, key, s);
        p.rng.ctr = ctr;
        p.o = mk3(a.x, a.y, a.z);
        // (GATHER) an irradiance query: the row is a point and b.xyz its normal - the sample draws its direction here, while only the row and
        // the generator are live, and the path goes on from the counter the draws leave
        p.d = GATHER ? irradiance_direction(P.mode, mk3(b.x, b.y, b.z), p.rng) : mk3(b.x, b.y, b.z);
        p.A = mk3(1.f, 1.f, 1.f);
        p.C = mk3(inf, inf, inf);
        p.acc_len = 0.0f;
        p.depth = 0;
        p.pdf_seen = false;
        p.from = 0u;
        tmin = a.w; tmax = b.w;  // the depth-0 search runs over the ray's own interval; every later one over [RAY_MIN, +inf)
        alive = true;
      }
      trav_restart_world<STRICT>(t, S, p.o, p.d, tmin, tmax, again);  // (again: a bound the needle rule had set for this ray stays)
      in_flight = true;
    }
    // ---- search: one step per turn for every lane that has one, until the wave votes to leave for the service block ----
#if SOL_LOOP_PRIO
    __builtin_amdgcn_s_setprio(SOL_LOOP_PRIO);
#endif
    for (;;) {
      const bool act = t.cur != REF_DONE;
      if (!wave_keeps_searching(act, P.switch_below)) break;
      trav_step_wave<false, false, STRICT>(S, t, act, st, p.rng, p.depth, cnt);
    }
#if SOL_LOOP_PRIO
    __builtin_amdgcn_s_setprio(0);
#endif
  }
