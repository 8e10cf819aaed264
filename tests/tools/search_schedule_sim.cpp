// search_schedule_sim.cpp -- CPU model of the search loop's SCHEDULE for one wave (not a pytest, no GPU): how many wave-level executions of
// the node part, the primitive part and the service block a sample costs under a given primitive-queue depth Q, primitive vote K
// (SOL_PRIM_MIN) and leave rule SW (switch_below), on the real C3 mesh. It models the schedule of sol_trace.h trav_step_wave, not its
// arithmetic: its tree, its materials and its camera are stand-ins, so its absolute counts are near the kernel's, not equal to them.
//
//   python tests/tools/dump_atrium_mesh.py /tmp/atrium.bin          (scenes.atrium_mesh as float32 [n][3][3])
//   g++ -O2 -std=c++17 tests/tools/search_schedule_sim.cpp -o /tmp/search_schedule_sim
//   /tmp/search_schedule_sim /tmp/atrium.bin [Q K SW]               (no Q K SW: the table of profiles/prim_queue_ab.txt)
//
// Tree: binned SAH (16 bins) binary tree, collapsed greedily (largest inner child first) into 7-wide nodes with single-triangle leaf
// slots; the hit inner children of a node are visited in the order of their centres along the ray's octant. Lanes: 64, one path each, C3's
// default camera; half of the bounces aim at the light quad, half are cosine-distributed; a path ends at a miss, at a direction below the
// surface or after 50 rays. Step: part 1 - every searching lane whose queue has room and which has a node group or a stack entry visits a
// node; the vote - the primitive part is skipped while fewer than K lanes hold a group and some lane can visit a node; part 2 - every
// holder tests ONE primitive of its oldest group. Service: a pass over the lanes whose search is over runs when fewer than SW lanes
// search (or none). Cost per sample: node part 153, primitive part 85, service pass 900 vector instructions per execution.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <deque>
#include <random>
#include <vector>

struct Vec { float x, y, z; };
static Vec operator-(Vec a, Vec b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
static Vec operator+(Vec a, Vec b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
static Vec operator*(Vec a, float s) { return {a.x * s, a.y * s, a.z * s}; }
static float dot(Vec a, Vec b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
static Vec cross(Vec a, Vec b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
static Vec unit(Vec a) { return a * (1.0f / std::sqrt(dot(a, a))); }
static float axis(const Vec& v, int a) { return a == 0 ? v.x : a == 1 ? v.y : v.z; }

struct Box {
  float lo[3] = {1e30f, 1e30f, 1e30f}, hi[3] = {-1e30f, -1e30f, -1e30f};
  void add(Vec p) { for (int a = 0; a < 3; ++a) { lo[a] = std::min(lo[a], axis(p, a)); hi[a] = std::max(hi[a], axis(p, a)); } }
  void add(const Box& b) { for (int a = 0; a < 3; ++a) { lo[a] = std::min(lo[a], b.lo[a]); hi[a] = std::max(hi[a], b.hi[a]); } }
  float area() const { const float d0 = hi[0] - lo[0], d1 = hi[1] - lo[1], d2 = hi[2] - lo[2]; return d0 * d1 + d1 * d2 + d2 * d0; }
  Vec centre() const { return {(lo[0] + hi[0]) * 0.5f, (lo[1] + hi[1]) * 0.5f, (lo[2] + hi[2]) * 0.5f}; }
};

// ---- the mesh and the two trees ----
static std::vector<Vec> verts;  // three per triangle
static std::vector<Box> tri_box;
static std::vector<Vec> tri_centre;
struct BinaryNode { Box box; int left = -1, right = -1, tri = -1; };
static std::vector<BinaryNode> binary;
struct WideNode { int n = 0; Box child_box[7]; int child[7]; Box box; };  // child >= 0: a wide node; < 0: ~triangle
static std::vector<WideNode> wide;

static int build_binary(std::vector<int>& idx, int lo, int hi) {
  constexpr int BINS = 16;
  BinaryNode node;
  Box centres;
  for (int i = lo; i < hi; ++i) { node.box.add(tri_box[idx[i]]); centres.add(tri_centre[idx[i]]); }
  const int me = (int)binary.size();
  binary.push_back(node);
  if (hi - lo == 1) { binary[me].tri = idx[lo]; return me; }
  int best_axis = -1, best_split = -1;
  float best_cost = 1e30f;
  auto bin_of = [&](int t, int a) { return std::min(BINS - 1, (int)((axis(tri_centre[t], a) - centres.lo[a]) / (centres.hi[a] - centres.lo[a]) * BINS)); };
  for (int a = 0; a < 3; ++a) {
    if (centres.hi[a] - centres.lo[a] <= 0.0f) continue;
    Box bins[BINS];
    int count[BINS] = {0};
    for (int i = lo; i < hi; ++i) { const int k = bin_of(idx[i], a); bins[k].add(tri_box[idx[i]]); count[k]++; }
    float right_area[BINS];
    int right_count[BINS];
    Box acc;
    int c = 0;
    for (int k = BINS - 1; k > 0; --k) { acc.add(bins[k]); c += count[k]; right_area[k] = acc.area(); right_count[k] = c; }
    acc = Box();
    c = 0;
    for (int k = 0; k < BINS - 1; ++k) {
      acc.add(bins[k]);
      c += count[k];
      if (c == 0 || right_count[k + 1] == 0) continue;
      const float cost = acc.area() * c + right_area[k + 1] * right_count[k + 1];
      if (cost < best_cost) { best_cost = cost; best_axis = a; best_split = k; }
    }
  }
  int mid = (lo + hi) / 2;
  if (best_axis >= 0) {
    const int m = (int)(std::partition(idx.begin() + lo, idx.begin() + hi, [&](int t) { return bin_of(t, best_axis) <= best_split; }) - idx.begin());
    if (m != lo && m != hi) mid = m;
  }
  const int l = build_binary(idx, lo, mid), r = build_binary(idx, mid, hi);
  binary[me].left = l;
  binary[me].right = r;
  return me;
}

static int collapse(int b) {
  std::vector<int> c = {binary[b].left, binary[b].right};
  while ((int)c.size() < 7) {  // open the inner child with the largest box
    int pick = -1;
    float pick_area = -1.0f;
    for (int i = 0; i < (int)c.size(); ++i)
      if (binary[c[i]].tri < 0 && binary[c[i]].box.area() > pick_area) { pick_area = binary[c[i]].box.area(); pick = i; }
    if (pick < 0) break;
    const int x = c[pick];
    c[pick] = binary[x].left;
    c.push_back(binary[x].right);
  }
  const int me = (int)wide.size();
  wide.push_back(WideNode());
  wide[me].n = (int)c.size();
  wide[me].box = binary[b].box;
  for (int i = 0; i < (int)c.size(); ++i) {
    Box bx = binary[c[i]].box;
    for (int a = 0; a < 3; ++a) { bx.lo[a] -= 1e-4f; bx.hi[a] += 1e-4f; }
    wide[me].child_box[i] = bx;
    const int v = binary[c[i]].tri >= 0 ? ~binary[c[i]].tri : collapse(c[i]);  // (may grow `wide`: no reference held across the call)
    wide[me].child[i] = v;
  }
  return me;
}

static bool triangle_hit(int t, Vec o, Vec d, float tmin, float tmax, float& tt) {
  const Vec v0 = verts[3 * t], e1 = verts[3 * t + 1] - v0, e2 = verts[3 * t + 2] - v0;
  const Vec pv = cross(d, e2);
  const float det = dot(e1, pv);
  if (std::fabs(det) < 1e-8f) return false;
  const float id = 1.0f / det;
  const Vec tv = o - v0;
  const float u = dot(tv, pv) * id;
  if (u < 0.0f || u > 1.0f) return false;
  const Vec q = cross(tv, e1);
  const float v = dot(d, q) * id;
  if (v < 0.0f || u + v > 1.0f) return false;
  tt = dot(e2, q) * id;
  return tt >= tmin && tt <= tmax;
}

// ---- one lane: a path and its search ----
struct Lane {
  Vec o, d, inv;
  float best = 1e30f;
  int hit = -1;
  std::vector<int> group;               // the node group: hit inner children of the node visited last, nearest first
  std::vector<std::vector<int>> stack;  // what was left of the groups above
  std::deque<std::vector<int>> held;    // primitive groups, oldest first
  bool searching = false, has_path = false;
  int depth = 0;
  bool can_descend() const { return !group.empty() || !stack.empty(); }
};

static std::mt19937 rng(1);
static std::uniform_real_distribution<float> uniform(0.0f, 1.0f);
static const Vec cam_from = {-13.0f, 2.2f, 0.6f}, cam_at = {6.0f, 4.5f, -0.4f};  // C3's default camera, vfov 55, 16:9
static Vec cam_w, cam_u, cam_v;
static float half_h, half_w;
static long long lane_visits, lane_prims, rays_done, samples_done;

static void start_ray(Lane& L, Vec o, Vec d) {
  L.o = o; L.d = d; L.inv = {1.0f / d.x, 1.0f / d.y, 1.0f / d.z};
  L.best = 1e30f; L.hit = -1;
  L.group.assign(1, 0);
  L.stack.clear();
  L.held.clear();
  L.searching = true;
}
static void camera_ray(Lane& L) {
  const float sx = (uniform(rng) * 2 - 1) * half_w, sy = (uniform(rng) * 2 - 1) * half_h;
  L.depth = 0;
  L.has_path = true;
  start_ray(L, cam_from, unit(cam_u * sx + cam_v * sy - cam_w));
}
// The lane's search is over: the next ray of its path, or the next sample.
static void service(Lane& L) {
  if (L.has_path) {
    rays_done++;
    if (L.hit >= 0 && L.depth < 49) {
      Vec n = unit(cross(verts[3 * L.hit + 1] - verts[3 * L.hit], verts[3 * L.hit + 2] - verts[3 * L.hit]));
      if (dot(n, L.d) > 0) n = n * -1.0f;
      const Vec hp = L.o + L.d * L.best;
      Vec nd;
      if (uniform(rng) < 0.5f) {  // towards the light quad above the roof opening
        nd = Vec{-6.0f + 12.0f * uniform(rng), 13.5f, -2.0f + 4.0f * uniform(rng)} - hp;
      } else {  // cosine-distributed
        Vec r;
        do { r = {uniform(rng) * 2 - 1, uniform(rng) * 2 - 1, uniform(rng) * 2 - 1}; } while (dot(r, r) >= 1 || dot(r, r) < 1e-6f);
        nd = n + unit(r);
        if (dot(nd, nd) < 1e-8f) nd = n;
      }
      if (dot(nd, n) > 0) { L.depth++; start_ray(L, hp, nd); return; }
    }
    samples_done++;
  }
  camera_ray(L);
}
static void visit(Lane& L) {
  if (L.group.empty()) { L.group = L.stack.back(); L.stack.pop_back(); }
  const int node = L.group.front();
  L.group.erase(L.group.begin());
  if (!L.group.empty()) L.stack.push_back(L.group);
  L.group.clear();
  lane_visits++;
  const WideNode& w = wide[node];
  const Vec nc = w.box.centre(), sign = {L.d.x < 0 ? -1.0f : 1.0f, L.d.y < 0 ? -1.0f : 1.0f, L.d.z < 0 ? -1.0f : 1.0f};
  std::vector<std::pair<float, int>> order;
  std::vector<int> prims;
  for (int i = 0; i < w.n; ++i) {
    float t0 = 1e-3f, t1 = L.best;
    for (int a = 0; a < 3; ++a) {
      float ta = (w.child_box[i].lo[a] - axis(L.o, a)) * axis(L.inv, a), tb = (w.child_box[i].hi[a] - axis(L.o, a)) * axis(L.inv, a);
      if (ta > tb) std::swap(ta, tb);
      t0 = std::max(t0, ta);
      t1 = std::min(t1, tb);
    }
    if (!(t0 <= t1)) continue;
    if (w.child[i] < 0) prims.push_back(~w.child[i]);
    else order.push_back({dot(w.child_box[i].centre() - nc, sign), w.child[i]});
  }
  std::sort(order.begin(), order.end());
  for (const auto& p : order) L.group.push_back(p.second);
  if (!prims.empty()) L.held.push_back(prims);
}
static void primitive_test(Lane& L) {
  const int t = L.held.front().front();
  L.held.front().erase(L.held.front().begin());
  if (L.held.front().empty()) L.held.pop_front();
  lane_prims++;
  float tt;
  if (triangle_hit(t, L.o, L.d, 1e-3f, L.best, tt)) { L.best = tt; L.hit = t; }
}

struct Result { double rays, visits_per_ray, prims_per_ray, node_execs, node_lanes, prim_execs, prim_lanes, service, cost; };
static Result run(int Q, int K, int SW, long long n_samples) {
  rng.seed(1);
  lane_visits = lane_prims = rays_done = samples_done = 0;
  std::vector<Lane> lanes(64);
  long long node_execs = 0, prim_execs = 0, service_execs = 0, node_lanes = 0, prim_lanes = 0;
  auto room = [&](const Lane& l) { return l.searching && (int)l.held.size() < Q && l.can_descend(); };
  while (samples_done < n_samples) {
    service_execs++;
    for (auto& l : lanes) if (!l.searching) service(l);
    for (;;) {
      int searching = 0;
      for (const auto& l : lanes) searching += l.searching;
      if (searching == 0 || (searching != 64 && searching < SW)) break;
      int visited = 0;  // part 1
      for (auto& l : lanes) if (room(l)) { visit(l); visited++; }
      if (visited) { node_execs++; node_lanes += visited; }
      int holders = 0, can_visit = 0;  // the vote
      for (auto& l : lanes) {
        if (!l.searching) continue;
        if (!l.held.empty()) holders++;
        else if (!l.can_descend()) l.searching = false;
        if (room(l)) can_visit++;
      }
      if (holders == 0 || (can_visit && holders < K)) continue;
      prim_execs++;  // part 2
      for (auto& l : lanes) {
        if (!l.searching || l.held.empty()) continue;
        primitive_test(l);
        prim_lanes++;
        if (l.held.empty() && !l.can_descend()) l.searching = false;
      }
    }
  }
  const double S = (double)samples_done;
  return {rays_done / S, (double)lane_visits / rays_done, (double)lane_prims / rays_done, node_execs / S, (double)node_lanes / node_execs,
          prim_execs / S, (double)prim_lanes / prim_execs, service_execs / S, (node_execs * 153.0 + prim_execs * 85.0 + service_execs * 900.0) / S};
}
static void print_row(int Q, int K, int SW, const Result& r) {
  std::printf("Q %d  K %2d  SW %2d | node parts / sample %.3f (lanes %.1f) | prim parts / sample %.3f (lanes %.1f) | service passes / sample %.4f | "
              "rays / sample %.2f  visits / ray %.2f  prims / ray %.2f | model cost / sample %.1f\n",
              Q, K, SW, r.node_execs, r.node_lanes, r.prim_execs, r.prim_lanes, r.service, r.rays, r.visits_per_ray, r.prims_per_ray, r.cost);
}

int main(int argc, char** argv) {
  if (argc != 2 && argc != 5) { std::fprintf(stderr, "usage: %s mesh.bin [Q K SW]\n", argv[0]); return 2; }
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) { std::perror(argv[1]); return 1; }
  std::fseek(f, 0, SEEK_END);
  const long bytes = std::ftell(f);
  std::fseek(f, 0, SEEK_SET);
  const int n_tri = (int)(bytes / 36);
  verts.resize((size_t)n_tri * 3);
  if (n_tri == 0 || std::fread(verts.data(), 36, n_tri, f) != (size_t)n_tri) { std::fprintf(stderr, "%s: short read\n", argv[1]); return 1; }
  std::fclose(f);
  tri_box.resize(n_tri);
  tri_centre.resize(n_tri);
  for (int t = 0; t < n_tri; ++t) {
    for (int k = 0; k < 3; ++k) tri_box[t].add(verts[3 * t + k]);
    tri_centre[t] = tri_box[t].centre();
  }
  std::vector<int> idx(n_tri);
  for (int i = 0; i < n_tri; ++i) idx[i] = i;
  binary.reserve(2 * (size_t)n_tri);
  build_binary(idx, 0, n_tri);
  wide.reserve(n_tri);
  collapse(0);
  cam_w = unit(cam_from - cam_at);
  cam_u = unit(cross(Vec{0, 1, 0}, cam_w));
  cam_v = cross(cam_w, cam_u);
  half_h = std::tan(55.0f * 3.14159265f / 360.0f);
  half_w = half_h * 1920.0f / 1080.0f;
  std::printf("%d triangles, %zu wide nodes\n", n_tri, wide.size());
  const long long n_samples = 300000;
  if (argc == 5) {
    const int Q = std::atoi(argv[2]), K = std::atoi(argv[3]), SW = std::atoi(argv[4]);
    print_row(Q, K, SW, run(Q, K, SW, n_samples));
    return 0;
  }
  const int table[][2] = {{1, 8}, {1, 12}, {2, 8}, {2, 12}, {2, 16}, {3, 8}};
  for (const auto& qk : table) print_row(qk[0], qk[1], 16, run(qk[0], qk[1], 16, n_samples));
  return 0;
}
