// The training MaxPool2d(2) window rule and the bilinear x2 source-index rule, each defined once for
// pool_up.hip and the conv epilogues that re-derive them (conv_igemm.hip's fused eval upsample).
#pragma once
#include "common.h"

// 2x2 window v[0..3] in row-major order: the FIRST maximum wins and a NaN beats everything, as torch's
// MaxPool2d forward / backward pair does. The eval conv epilogues pool with fmaxf instead (NaN loses):
// a different rule on purpose, not an instance of this one. maxpool2_bwd and the two fused pool kernels of
// pool_up.hip keep hand-written copies of this rule (marked in place: the shared form measured slower there).
RDP_DEV float max4(float v0, float v1, float v2, float v3) {
  float m = v0;
  if (v1 > m || isnan(v1)) m = v1;
  if (v2 > m || isnan(v2)) m = v2;
  if (v3 > m || isnan(v3)) m = v3;
  return m;
}

// align_corners=True source of output index u: s = r * u in fp32 (r = (in - 1) / (out - 1)), taps i0 and
// i1 = i0 + (i0 < in - 1), weight l1 on i1 (torch area_pixel_compute_source_index)
RDP_DEV void up_src(int u, int in, float r, int& i0, int& i1, float& l1) {
  const float s = r * (float)u;
  i0 = (int)s;
  i1 = i0 + (i0 < in - 1 ? 1 : 0);
  l1 = s - (float)i0;
}
