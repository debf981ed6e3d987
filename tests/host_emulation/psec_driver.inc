// appended to a system's Poincare-section companion source (System.poincare_source): run hamk_psec_steps_k for every (block,
// thread) on the host, as driver.inc does for the kernels of the per-system module
extern "C" {
void emu_psec(double* q, double* p, long long B, double dt, int nsteps, int coord, double level, double period, int direction,
              int max_hits, double* qhit, double* phit, double* thit, int* nhit, long long step0, int* status) {
  blockDim.x = 256;
  for (long long b0 = 0; b0 < B; b0 += 256) {
    blockIdx.x = (unsigned)(b0 / 256);
    for (unsigned t = 0; t < 256; ++t) {
      threadIdx.x = t;
      hamk_psec_steps_k(q, p, B, dt, nsteps, coord, level, period, direction, max_hits, qhit, phit, thit, nhit, step0, status);
    }
  }
}
}
