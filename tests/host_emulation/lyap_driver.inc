// appended to a system's Lyapunov companion source (System.lyapunov_source): run hamk_lyap_steps_k for every (block, thread)
// on the host, as driver.inc does for the kernels of the per-system module
extern "C" {
void emu_lyap(double* q, double* p, double* wq, double* wp, long long B, double dt, int nintervals, int every, double d0,
              double* logsum, int* status) {
  blockDim.x = 256;
  for (long long b0 = 0; b0 < B; b0 += 256) {
    blockIdx.x = (unsigned)(b0 / 256);
    for (unsigned t = 0; t < 256; ++t) {
      threadIdx.x = t;
      hamk_lyap_steps_k(q, p, wq, wp, B, dt, nintervals, every, d0, logsum, status);
    }
  }
}
}
