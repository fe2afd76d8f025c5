// Accuracy of the fast-math intrinsics the loss heads use, measured alone against fp64 on the host:
// __expf over [-80, 0] (the heads call it on -|x| and on x - max), log1pf(e) for e = exp(-|x|), logf over
// [1, 8] (the K-class sum of exponentials) and the fp32 division 1 / (1 + e). Not a head kernel: one
// elementwise kernel per function. Prints the worst relative error of each in units of 2^-24 (the fp32
// unit roundoff), which tests/test_head_exact_gpu.py doubles for its allowance (profiles/head_exact.md).
//
//   hipcc --offload-arch=gfx950 -O3 -ffp-contract=fast scripts/expf_probe.hip -o scripts/expf_probe
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <vector>

#define CHECK(e) do { hipError_t r_ = (e); if (r_ != hipSuccess) { printf("hip error %s at line %d\n", hipGetErrorString(r_), __LINE__); return 1; } } while (0)

__global__ void probe_kernel(const float* __restrict__ x, float* __restrict__ out, int n, int fn) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float v = x[i];
  float r;
  if (fn == 0) r = __expf(v);
  else if (fn == 1) r = log1pf(v);
  else if (fn == 2) r = logf(v);
  else r = 1.f / (1.f + v);
  out[i] = r;
}

static int run(const char* name, int fn, const std::vector<float>& x, double (*ref)(double)) {
  const int n = (int)x.size();
  float *dx, *dout;
  CHECK(hipMalloc(&dx, n * sizeof(float)));
  CHECK(hipMalloc(&dout, n * sizeof(float)));
  CHECK(hipMemcpy(dx, x.data(), n * sizeof(float), hipMemcpyHostToDevice));
  hipLaunchKernelGGL(probe_kernel, dim3((n + 255) / 256), dim3(256), 0, 0, dx, dout, n, fn);
  CHECK(hipGetLastError());
  std::vector<float> out(n);
  CHECK(hipMemcpy(out.data(), dout, n * sizeof(float), hipMemcpyDeviceToHost));
  double worst = 0.0, at = 0.0, wabs = 0.0;
  for (int i = 0; i < n; ++i) {
    const double r = ref((double)x[i]);
    const double d = std::fabs((double)out[i] - r);
    if (d > wabs) wabs = d;
    if (r == 0.0) continue;
    if (d / std::fabs(r) > worst) { worst = d / std::fabs(r); at = x[i]; }
  }
  printf("%-22s n=%d  max rel err = %.3e = %.3f x 2^-24 (at %.9g)  max abs err = %.3e = %.3f x 2^-24\n", name, n,
         worst, worst * 16777216.0, at, wabs, wabs * 16777216.0);
  if (fn == 0) {  // __expf's error grows with |x| (the product x * log2(e) rounds): worst per bucket of |x|
    const float edge[] = {0.f, 1.f, 2.f, 4.f, 8.f, 16.f, 32.f, 48.f, 80.f};
    double wb[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int i = 0; i < n; ++i) {
      const double r = ref((double)x[i]);
      const double e = std::fabs((double)out[i] - r) / r;
      int b = 0;
      while (b < 7 && std::fabs(x[i]) > edge[b + 1]) ++b;
      if (e > wb[b]) wb[b] = e;
    }
    for (int b = 0; b < 8; ++b)
      printf("    |x| in (%g, %g]: max rel err = %.3f x 2^-24\n", edge[b], edge[b + 1], wb[b] * 16777216.0);
  }
  CHECK(hipFree(dx));
  CHECK(hipFree(dout));
  return 0;
}

static double ref_exp(double v) { return std::exp(v); }
static double ref_log1p(double v) { return std::log1p(v); }
static double ref_log(double v) { return std::log(v); }
static double ref_rcp1p(double v) { return 1.0 / (1.0 + v); }

int main() {
  const int N = 1 << 21;
  std::vector<float> xe, xl, xs;
  for (int i = 0; i <= N; ++i) xe.push_back(-80.f * (float)i / (float)N);   // dense
  for (int i = 0; i <= 8 * 80; ++i) xe.push_back(-(float)i / 8.f);          // the lattice logits' own values
  std::vector<float> xe45;
  for (float v : xe) if (v >= -45.f) xe45.push_back(v);
  for (float v : xe45) xl.push_back((float)std::exp((double)v));            // e = exp(-|x|) in (0, 1]
  for (int i = 0; i <= N; ++i) xs.push_back(1.f + 7.f * (float)i / (float)N);
  if (run("__expf [-45, 0]", 0, xe45, ref_exp)) return 1;
  if (run("__expf [-80, 0]", 0, xe, ref_exp)) return 1;
  if (run("log1pf(e), e in (0,1]", 1, xl, ref_log1p)) return 1;
  if (run("logf [1, 8]", 2, xs, ref_log)) return 1;
  if (run("1 / (1 + e)", 3, xl, ref_rcp1p)) return 1;
  return 0;
}
