// appended to a system's symplectic companion source (System.symplectic_source): run hamk_symp_steps_k for every (block, thread)
// on the host, as driver.inc does for the kernels of the per-system module
extern "C" {
void emu_symp(double* q, double* p, long long B, int nsteps, int nsub, double ha, double hb, int iters, double* residual, int* status) {
  blockDim.x = 256;
  for (long long b0 = 0; b0 < B; b0 += 256) {
    blockIdx.x = (unsigned)(b0 / 256);
    for (unsigned t = 0; t < 256; ++t) {
      threadIdx.x = t;
      hamk_symp_steps_k(q, p, B, nsteps, nsub, ha, hb, iters, residual, status);
    }
  }
}
}
