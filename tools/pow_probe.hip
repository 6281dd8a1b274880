// Device pow(x, beta) with beta a kernel argument, as es_reduce_kernel calls it, over a file of
// doubles: the figure behind tests/block_cases.py POW_MEASURED_ULP["device"].
//   hipcc -O3 --offload-arch=gfx950 tools/pow_probe.hip -o tools/pow_probe
//   tools/pow_probe in.bin out.bin beta [beta ...]     (out: one block of n doubles per beta)
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <vector>

__global__ void pow_kernel(const double* __restrict__ x, int n, double beta, double* __restrict__ y) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) y[i] = pow(x[i], beta);
}

#define CHK(e)                                                        \
  do {                                                                \
    hipError_t r_ = (e);                                              \
    if (r_ != hipSuccess) {                                           \
      fprintf(stderr, "%s: %s\n", #e, hipGetErrorString(r_));         \
      return 1;                                                       \
    }                                                                 \
  } while (0)

int main(int argc, char** argv) {
  if (argc < 4) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  std::vector<double> x;
  double v;
  while (fread(&v, 8, 1, f) == 1) x.push_back(v);
  fclose(f);
  const int n = (int)x.size();
  if (n == 0) return 2;
  double *dx, *dy;
  CHK(hipMalloc(&dx, (size_t)n * 8));
  CHK(hipMalloc(&dy, (size_t)n * 8));
  CHK(hipMemcpy(dx, x.data(), (size_t)n * 8, hipMemcpyHostToDevice));
  FILE* o = fopen(argv[2], "wb");
  if (!o) return 2;
  std::vector<double> y(n);
  for (int a = 3; a < argc; ++a) {
    hipLaunchKernelGGL(pow_kernel, dim3((n + 255) / 256), dim3(256), 0, 0, dx, n, atof(argv[a]), dy);
    CHK(hipGetLastError());
    CHK(hipMemcpy(y.data(), dy, (size_t)n * 8, hipMemcpyDeviceToHost));
    fwrite(y.data(), 8, n, o);
  }
  fclose(o);
  printf("pow_probe: %d values, %d exponents\n", n, argc - 3);
  return 0;
}
