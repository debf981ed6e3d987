// codegen_threads.cpp -- generate_source from two threads at once (include/hamk.h: distinct handles may be used concurrently, and every
// handle generates its sources lazily).  Built with hamk_codegen.cpp under -fsanitize=thread by tests/test_codegen_threads.py.
// Two systems whose emitted text depends on what generate_source tells emit_body about the tape:
//   dense   four lanes per trajectory, quad_dense, n = 18: x_k = 2 q_k + sum_j a_j sin q_j + b_j cos q_j with the products a_j sin q_j,
//           b_j cos q_j shared by all outputs -- written out at every use (opaque_const) only while the unshare flag is on
//   lane    n = 2 with U = 1 / sqrt(1 + q0^2 + q1^2): RECIP(SQRT(.)) is fused into rsqrt_of only while the square root is no output
// Each source is generated once alone, then both are generated concurrently in a loop: every result must equal the first.
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <thread>

#include "hamk_internal.h"

using namespace hamk_host;

namespace {
struct Tape {
  std::vector<hamk_op> ops;
  int add(int op, int a = 0, int b = 0, double c = 0.0) {
    hamk_op o{};
    o.op = op; o.a = a; o.b = b; o.c = c;
    ops.push_back(o);
    return (int)ops.size() - 1;
  }
};

SystemDesc dense_quad() {
  const int n = 18;
  SystemDesc d;
  d.m = n; d.n = n; d.u_space = HAMK_U_GENERALIZED;
  d.mode_h = false; d.mode_r = true; d.rk4_stage_loop = true; d.rkf_stage_loop = true;
  d.mapping = HAMK_MAP_QUAD; d.quad_dense = true; d.rkf_park = true; d.k_symbolic = false; d.use_lut = 0;
  d.inertia.assign(n, 1.0);
  Tape f;
  std::vector<int> q(n), as(n), bc(n);
  for (int j = 0; j < n; ++j) q[j] = f.add(HAMK_OP_INPUT, j);
  for (int j = 0; j < n; ++j) {
    as[j] = f.add(HAMK_OP_MUL, f.add(HAMK_OP_CONST, 0, 0, 0.2 + 0.01 * j), f.add(HAMK_OP_SIN, q[j]));
    bc[j] = f.add(HAMK_OP_MUL, f.add(HAMK_OP_CONST, 0, 0, 0.15 + 0.01 * j), f.add(HAMK_OP_COS, q[j]));
  }
  for (int k = 0; k < n; ++k) {
    int x = f.add(HAMK_OP_MUL, f.add(HAMK_OP_CONST, 0, 0, 2.0), q[k]);
    for (int j = 0; j < n; ++j) x = f.add(HAMK_OP_ADD, f.add(HAMK_OP_ADD, x, as[j]), bc[j]);
    d.f_outs.push_back(x);
  }
  d.f_ops = f.ops;
  Tape u;
  int acc = -1;
  for (int j = 0; j < n; ++j) {
    const int qj = u.add(HAMK_OP_INPUT, j), sq = u.add(HAMK_OP_MUL, qj, qj);
    acc = acc < 0 ? sq : u.add(HAMK_OP_ADD, acc, sq);
  }
  d.u_ops = u.ops; d.u_out = acc;
  return d;
}

SystemDesc lane_rsqrt() {
  SystemDesc d;
  d.m = 2; d.n = 2; d.u_space = HAMK_U_GENERALIZED;
  d.mapping = HAMK_MAP_LANE; d.k_symbolic = false;
  d.inertia.assign(2, 1.0);
  Tape f;
  for (int j = 0; j < 2; ++j) d.f_outs.push_back(f.add(HAMK_OP_MUL, f.add(HAMK_OP_CONST, 0, 0, 1.5), f.add(HAMK_OP_INPUT, j)));
  d.f_ops = f.ops;
  Tape u;
  const int q0 = u.add(HAMK_OP_INPUT, 0), q1 = u.add(HAMK_OP_INPUT, 1);
  const int r2 = u.add(HAMK_OP_ADD, u.add(HAMK_OP_ADD, u.add(HAMK_OP_CONST, 0, 0, 1.0), u.add(HAMK_OP_MUL, q0, q0)), u.add(HAMK_OP_MUL, q1, q1));
  d.u_out = u.add(HAMK_OP_RECIP, u.add(HAMK_OP_SQRT, r2));
  d.u_ops = u.ops;
  return d;
}

bool valid(const SystemDesc& d) {
  return validate_tape(d.f_ops.data(), (int)d.f_ops.size(), d.n, d.f_outs.data(), d.m, "f").empty() &&
         validate_tape(d.u_ops.data(), (int)d.u_ops.size(), d.n, &d.u_out, 1, "u").empty();
}
}  // namespace

int main(int argc, char** argv) {
  const int rounds = argc > 1 ? std::atoi(argv[1]) : 20;
  const SystemDesc sys[2] = {dense_quad(), lane_rsqrt()};
  if (!valid(sys[0]) || !valid(sys[1])) { std::fprintf(stderr, "a hand-built tape is invalid\n"); return 2; }
  const std::string alone[2] = {generate_source(sys[0]), generate_source(sys[1])};
  // the two properties the systems were built for are in the text at all
  if (alone[0].find("hamk::opaque_const(") == std::string::npos || alone[1].find("hamk::rsqrt_of(") == std::string::npos ||
      alone[1].find("hamk::opaque_const(") != std::string::npos) {
    std::fprintf(stderr, "the sources do not show the unshared scales / the fused 1 / sqrt\n");
    return 2;
  }
  // the dense source takes many times longer than the lane one: the lane thread keeps generating until the dense thread is through
  int differ[2] = {0, 0}, lane_rounds = 0;
  std::atomic<bool> dense_done{false};
  std::thread a([&] { for (int r = 0; r < rounds; ++r) if (generate_source(sys[0]) != alone[0]) ++differ[0]; dense_done = true; });
  std::thread b([&] { do { if (generate_source(sys[1]) != alone[1]) ++differ[1]; ++lane_rounds; } while (!dense_done); });
  a.join(); b.join();
  std::printf("dense: %d rounds, %d differ; lane: %d rounds, %d differ\n", rounds, differ[0], lane_rounds, differ[1]);
  return (differ[0] || differ[1]) ? 1 : 0;
}
