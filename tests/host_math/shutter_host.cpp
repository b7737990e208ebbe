// TEST INFRASTRUCTURE ONLY: the time tangent of the screw interpolation (gs_math.h::subpose_tangent_dot, the per-item
// arithmetic of subpose_bwd_kernel) compiled for the host with g++, so that d loss / d sub-pose time can be checked against
// float64 autograd through matrix_exp on a machine without a GPU.  Never loaded by the product package.
#include "gs_math.h"
using namespace gs;

extern "C" {

// what gs_subpose_viewmats_bwd_times computes, item by item in the kernel's order: the 18 camera tangents summed over the
// sub-poses in order (v_V0[16] row 3 = 0, v_lin[3], v_ang[3]) and the time tangent of every sub-pose (v_times[P])
int sh_subpose_bwd_times(int P, const float* V0, const float* lin, const float* ang, const float* times,
                         const float* v_out /*P*16*/, float* v_V0 /*16*/, float* v_lin, float* v_ang, float* v_times) {
  float sum[18];
  for (int t = 0; t < 18; ++t) sum[t] = 0.f;
  for (int p = 0; p < P; ++p) {
    for (int t = 0; t < 18; ++t) sum[t] += subpose_tangent_dot(V0, lin, ang, times[p], v_out + 16 * p, t);
    v_times[p] = subpose_tangent_dot(V0, lin, ang, times[p], v_out + 16 * p, 18);
  }
  for (int t = 0; t < 12; ++t) v_V0[t] = sum[t];
  for (int t = 12; t < 16; ++t) v_V0[t] = 0.f;
  for (int t = 0; t < 3; ++t) { v_lin[t] = sum[12 + t]; v_ang[t] = sum[15 + t]; }
  return 0;
}

// the closed form -<v_out_p, xi^ V_p> on the float32 sub-pose matrices
int sh_subpose_time_closed(int P, const float* V0, const float* lin, const float* ang, const float* times,
                           const float* v_out /*P*16*/, float* v_times) {
  for (int p = 0; p < P; ++p) {
    float Vp[12];
    subpose_viewmat<float>(V0, lin, ang, times[p], Vp);
    v_times[p] = subpose_time_dot_closed(Vp, lin, ang, v_out + 16 * p);
  }
  return 0;
}

}  // extern "C"
