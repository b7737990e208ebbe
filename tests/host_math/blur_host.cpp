// TEST INFRASTRUCTURE ONLY: csrc/blur_math.h compiled for the host (tests/test_blur_host.py).  The per-pair function, the
// partial sums and the final division are the kernels'; the pairs of a frame are added one after the other here.
#include "blur_math.h"

namespace bl = gs::blur;

extern "C" {

int bh_chunk() { return bl::kChunk; }
int bh_frame_group() { return bl::kFrameGroup; }
float bh_default_clip() { return bl::kDefaultClip; }

// one pair: -> visible (0 / 1), out[0] = blur, out[1] = skew
int bh_pair(const float* p, const float* V, const float* lin, const float* ang, const float* intrins, const float* times,
            int W, int H, float clip, float* out) {
  const bl::Frame fr = {V, lin, ang, intrins[0], intrins[1], intrins[2], intrins[3], times[0], times[1]};
  return bl::pair_blur(fr, p, (float)W, (float)H, clip, out, out + 1) ? 1 : 0;
}

// the arguments of gs_blur_stats, host pointers
void bh_blur_stats(int F, int N, const float* points, const float* viewmats, const float* lin, const float* ang,
                   const float* intrins, const float* times, int W, int H, float clip, int* counts, float* stats) {
  for (int f = 0; f < F; ++f) {
    const bl::Frame fr = {viewmats + (size_t)f * 16, lin + (size_t)f * 3, ang + (size_t)f * 3, intrins[f * 4],
                          intrins[f * 4 + 1], intrins[f * 4 + 2], intrins[f * 4 + 3], times[f * 2], times[f * 2 + 1]};
    bl::Partial a;
    bl::clear_partial(a);
    for (int i = 0; i < N; ++i) {
      float blur, skew;
      const bool visible = bl::pair_blur(fr, points + (size_t)i * 3, (float)W, (float)H, clip, &blur, &skew);
      bl::add_pair(a, visible, blur, skew);
    }
    bl::finish(a, counts + f, stats + (size_t)f * 4);
  }
}

}  // extern "C"
