// Stand-alone check of the pure host helpers in sdslam_amd/csrc/orb_internal.h (no HIP call is made, nothing is linked from the
// HIP runtime): the graph cache key and the enumerations of the handle's events and buffers.  Built with
// -fsanitize=address,undefined by tests/test_host_cpu.py.
#define __HIP_PLATFORM_AMD__ 1
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <set>

#include "../../sdslam_amd/csrc/orb_internal.h"

#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); std::exit(1); } } while (0)

static bool inside(const sd_orb* h, const void* p) {
  return (const char*)p >= (const char*)h && (const char*)p < (const char*)(h + 1);
}

int main() {
  std::unique_ptr<sd_orb> hp(new sd_orb()), gp(new sd_orb());
  sd_orb *h = hp.get(), *g = gp.get();

  // graph key: every argument and the output set take part; the distortion values only while distortion is on
  int frames = 0;
  h->set = g->set = 1;
  const sd_orb::GraphKey k0 = graph_key(h, &frames, 4, 640, 640 * 480);
  CHECK(k0 == graph_key(g, &frames, 4, 640, 640 * 480));
  CHECK(!(k0 == graph_key(h, &frames + 1, 4, 640, 640 * 480)));
  CHECK(!(k0 == graph_key(h, &frames, 3, 640, 640 * 480)));
  CHECK(!(k0 == graph_key(h, &frames, 4, 648, 640 * 480)));
  CHECK(!(k0 == graph_key(h, &frames, 4, 640, 648 * 480)));
  CHECK(!(k0 == sd_orb::GraphKey()));
  g->set = 0;
  CHECK(!(k0 == graph_key(g, &frames, 4, 640, 640 * 480)));
  g->set = 1;
  g->dist_K[0] = 500.f;
  g->dist[1] = 0.1f;   // k2 alone: have_dist stays off
  CHECK(k0 == graph_key(g, &frames, 4, 640, 640 * 480));
  g->have_dist = true;
  CHECK(!(k0 == graph_key(g, &frames, 4, 640, 640 * 480)));
  *h = sd_orb();
  h->set = 1;
  h->have_dist = true;
  h->dist_K[0] = 500.f;
  h->dist[1] = 0.1f;
  CHECK(graph_key(h, &frames, 4, 640, 640 * 480) == graph_key(g, &frames, 4, 640, 640 * 480));
  for (int i = 0; i < 9; i++) {
    float& v = i < 4 ? h->dist_K[i] : h->dist[i - 4];
    const float keep = v;
    v = keep + 1.f;
    CHECK(!(graph_key(h, &frames, 4, 640, 640 * 480) == graph_key(g, &frames, 4, 640, 640 * 480)));
    v = keep;
  }
  sd_orb::GraphEntry e;
  e.key = k0;
  CHECK(e.key == k0 && e.exec == nullptr);

  // events: every untimed event of the handle exactly once, the lazily created fence events not at all
  *h = sd_orb();
  std::set<const void*> seen;
  int marker = 0;
  const void *first = nullptr, *last = nullptr;
  for_each_event(h, [&](hipEvent_t& ev) {
    CHECK(inside(h, &ev) && ev == nullptr);
    CHECK(seen.insert(&ev).second);
    if (!first) first = &ev;
    last = &ev;
    ev = (hipEvent_t)&marker;
  });
  CHECK(seen.size() == 2 + 1 + SD_MAX_LEVELS + 5);
  CHECK(first == &h->ev_set_free[0] && last == &h->ev_blur_done);   // creation order
  CHECK(h->ev_set_free[0] && h->ev_set_free[1] && h->ev_extract_done && h->ev_fast_done && h->ev_select_done && h->ev_body_start &&
        h->ev_pyr_done && h->ev_blur_done);
  for (hipEvent_t ev : h->ev_level) CHECK(ev);
  CHECK(!h->ev_user_fence[0] && !h->ev_user_fence[1] && !h->ev[0][0] && !h->evf[0][0]);

  // buffers: two disjoint lists of distinct pointer fields; clearing one list leaves the other alone
  *h = sd_orb();
  seen.clear();
  for (void** p : geom_buffers(h)) {
    CHECK(inside(h, p) && *p == nullptr && seen.insert(p).second);
    *p = &marker;
  }
  CHECK(h->d_cells && h->d_tiles && h->d_coef && h->pyr_set[0] && h->pyr_set[1] && h->d_blur && h->d_cand && h->d_scratch &&
        h->d_cell_count && h->d_sel && h->d_sel_count && h->d_cell_keep && h->d_cell_off && h->d_lvl_m);
  CHECK(!h->d_plan && !h->d_img && !h->kps_set[0] && !h->nout_set[1]);
  for (void** p : fixed_buffers(h)) {
    CHECK(inside(h, p) && *p == nullptr && seen.insert(p).second);
    *p = &marker;
  }
  CHECK(seen.size() == 24);
  CHECK(h->d_plan && h->d_img && h->kps_set[0] && h->kps_set[1] && h->kps_un_set[0] && h->kps_un_set[1] && h->desc_set[0] &&
        h->desc_set[1] && h->nout_set[0] && h->nout_set[1]);
  for (void** p : geom_buffers(h)) *p = nullptr;
  CHECK(!h->d_cells && !h->d_lvl_m && h->d_plan && h->nout_set[1]);
  select_set(h, 1);
  CHECK(h->set == 1 && h->d_pyr == h->pyr_set[1] && h->d_kps == h->kps_set[1] && h->d_nout == h->nout_set[1]);
  std::printf("orb_host_check OK\n");
  return 0;
}
