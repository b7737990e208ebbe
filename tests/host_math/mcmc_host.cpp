// TEST INFRASTRUCTURE ONLY: csrc/mcmc_math.h compiled for the host (tests/test_mcmc_host.py).
#include "mcmc_math.h"

extern "C" {

void mh_philox(const uint32_t* counter, const uint32_t* key, uint32_t* out) {
  uint32_t c[4] = {counter[0], counter[1], counter[2], counter[3]};
  gs::mcmc::philox4x32_10(c, key[0], key[1]);
  for (int i = 0; i < 4; ++i) out[i] = c[i];
}

void mh_row_words(int n, unsigned long long seed, unsigned long long step, uint32_t* words) {
  for (int r = 0; r < n; ++r) gs::mcmc::row_words((uint32_t)r, seed, step, words + 4 * (size_t)r);
}

void mh_normals(int n, const uint32_t* words, float* z) {
  for (int r = 0; r < n; ++r) gs::mcmc::normals3(words + 4 * (size_t)r, z + 3 * (size_t)r);
}

void mh_noise_delta(int n, const float* log_scales, const float* quats, const float* logits, const float* z,
                    float scaler, float* delta) {
  for (int r = 0; r < n; ++r)
    gs::mcmc::noise_delta(log_scales + 3 * (size_t)r, quats + 4 * (size_t)r, logits[r], z + 3 * (size_t)r, scaler,
                          delta + 3 * (size_t)r);
}

void mh_relocation(int m, const float* opacities, const float* scales, const int* ratios, float* new_opacities,
                   float* new_scales) {
  for (int r = 0; r < m; ++r)
    gs::mcmc::relocation(opacities[r], scales + 3 * (size_t)r, ratios[r], new_opacities + r, new_scales + 3 * (size_t)r);
}

}  // extern "C"
