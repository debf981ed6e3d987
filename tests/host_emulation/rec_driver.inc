// appended to a system's recording companion source (System.record_source): run hamk_rec_steps_k for every (block, thread)
// on the host, as driver.inc does for the kernels of the per-system module
extern "C" {
void emu_rec(double* q, double* p, long long B, double dt, int nsteps, int every, int max_rows, double* qout, double* pout,
             double* hout, long long step0, long long row_base, int* status) {
  blockDim.x = 256;
  for (long long b0 = 0; b0 < B; b0 += 256) {
    blockIdx.x = (unsigned)(b0 / 256);
    for (unsigned t = 0; t < 256; ++t) {
      threadIdx.x = t;
      hamk_rec_steps_k(q, p, B, dt, nsteps, every, max_rows, qout, pout, hout, step0, row_base, status);
    }
  }
}
}
