// The host build of a system's exit-time companion module (System.exit_source, written beside this text as exit_module.inc): run
// hamk_exit_steps_k for every (block, thread) on the host, as driver.inc does for the kernels of the per-system module.
// The device code runs thread by thread, so a wavefront is one thread and __ballot is the thread's own predicate: the step loop
// ends where THIS lane has stopped.  What the wave-wide break does to the other lanes only the GPU shows (tests/test_gpu_exit.py).
static inline unsigned long long __ballot(int predicate) { return predicate ? 1ull : 0ull; }
#include "exit_module.inc"
extern "C" {
void emu_exit(double* q, double* p, long long B, double dt, int nsteps, const int* coord, const double* lo, const double* hi, int ngates,
              int* code, double* texit, double* qexit, double* pexit, long long step0, int* status) {
  HamkGates gates;
  std::memset(&gates, 0, sizeof gates);
  for (int g = 0; g < 4; ++g) {
    gates.coord[g] = g < ngates ? coord[g] : 0;
    gates.lo[g] = g < ngates ? lo[g] : -HUGE_VAL;
    gates.hi[g] = g < ngates ? hi[g] : HUGE_VAL;
  }
  gates.ngates = ngates;
  blockDim.x = 256;
  for (long long b0 = 0; b0 < B; b0 += 256) {
    blockIdx.x = (unsigned)(b0 / 256);
    for (unsigned t = 0; t < 256; ++t) {
      threadIdx.x = t;
      hamk_exit_steps_k(q, p, B, dt, nsteps, gates, code, texit, qexit, pexit, step0, status);
    }
  }
}
}
