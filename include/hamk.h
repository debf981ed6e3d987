/*
 * hamk.h -- C ABI of libhamk.so: the MI355X (gfx950) replacement for the
 * equations-of-motion hot path of mstksg/hamilton (Numeric.Hamilton).
 *
 * Everything the reference does between "user hands over coordinate map f and
 * potential U" and "here is the next Phase" is behind these entry points:
 *
 *   reference (src/Numeric/Hamilton.hs)                 this ABI
 *   -------------------------------------------------   -------------------------
 *   mkSystem  :201-225 / mkSystem' :238-254             hamk_system_create
 *   System record :160-169 (opaque, GC-owned)           hamk_system (opaque handle) / hamk_system_destroy
 *   underlyingPos :174-178                              hamk_coords_batch
 *   pe            :182-186                              hamk_observe_batch (pe output)
 *   momenta :262-269, toPhase :279-284                  hamk_to_phase_batch
 *   velocities :316-324, fromPhase :332-337             hamk_from_phase_batch
 *   keC :288-296, lagrangian :301-309                   hamk_observe_config_batch
 *   keP :341-349, hamiltonian :353-361                  hamk_observe_batch
 *   hamEqs :370-387                                     hamk_hameqs_batch
 *   stepHam :390-402                                    hamk_step_ham_batch   (adaptive RKF45, GSL semantics)
 *   iterate (stepHam dt)  README.md:150, Examples.hs:429 hamk_step_ham_iterate (ncalls calls, one launch)
 *   evolveHam :433-462, evolveHam' :409-429             hamk_evolve_ham_batch (adaptive RKF45, GSL semantics)
 *   odeSolveV's GSL binding (:445, hmatrix-gsl)         hamk_system_set_gsl_api (gsl_odeiv2 driver | old gsl_odeiv)
 *   (no counterpart; named by BASELINE.json north_star) hamk_rk4_steps        (classic fixed-step RK4)
 *   (no counterpart)            hamk_rk4_steps_checked, hamk_checkpoint_*
 *   (no counterpart; a structure-preserving fixed step) hamk_symplectic_steps (implicit midpoint, order 2 / 4)
 *   (no counterpart; which trajectories are chaotic)    hamk_lyapunov_steps   (largest Lyapunov exponent, fused with RK4)
 *   (no counterpart; the surface of section)            hamk_poincare_steps   (crossings recorded inside a fused RK4 launch)
 *   (no counterpart; first-exit times)                  hamk_exit_steps       (when and where a trajectory leaves a box; it then stops)
 *   evolveHam's rows :433-462, on a fixed step          hamk_record_steps     (state / Hamiltonian rows recorded inside a fused RK4 launch)
 *
 * The reference evaluates ONE trajectory per call on the CPU through `ad`
 * (AD), hmatrix (LAPACK/BLAS) and hmatrix-gsl (GSL odeiv).  This library
 * evaluates an ENSEMBLE of B independent trajectories per call on the GPU:
 * one trajectory per wavefront lane up to n = 16, four lanes per trajectory
 * (sparse coordinate maps up to n = 32, and small ensembles of mid-size
 * systems) or 16 / 32 / 64 lanes per trajectory beyond -- chosen per launch
 * from (n, B), see hamk_options::mapping.  B = 1 reproduces the reference API.
 *
 * Data layout: every state array is structure-of-arrays, fp64, component
 * major: q[j*B + i] is generalized coordinate j of trajectory i (j < n,
 * i < B).  Arrays are caller-owned; nothing is retained after return.
 * `mem` says where the caller's pointers live: HAMK_MEM_HOST (PCIe-inclusive:
 * small arrays go through a pinned arena the kernel reads and writes directly,
 * large ones are staged through device memory; the call returns when the
 * results are in the caller's arrays) or HAMK_MEM_DEVICE (pointers are HIP
 * device pointers on the current device -- from the host's own runtime or from
 * hamk_device_malloc; the launch is asynchronous on the handle's stream, see
 * hamk_set_stream).
 *
 * User functions cross the ABI as expression tapes (hamk_op[]): the host
 * shim instantiates the reference's rank-2 polymorphic functions
 * (`forall a. RealFloat a => Vector n a -> Vector m a`, Hamilton.hs:212,215)
 * at a recording number type and ships the recording.  The library
 * specialises its hand-written device kernels on the tape at
 * hamk_system_create time (hiprtc, gfx950) -- the device-side AD that
 * replaces `jacobianT`/`hessianF`/`grad` (Hamilton.hs:221-224).
 *
 * Error convention: every entry point returns 0 on success, <0 on API /
 * toolchain / HIP failure (text via hamk_last_error(), thread-local).  This
 * replaces the reference's `error`/`fromJust`/hmatrix exceptions
 * (Hamilton.hs:425,444,462,321,381).  Numerical trouble is per trajectory in
 * status[B] (bit mask, HAMK_ST_*), never an exception.
 *
 * Threading: one handle is used by one host thread at a time; distinct
 * handles may be used concurrently.  A handle runs on the device that is
 * current (hamk_set_device) when it is first used; one handle per device is the
 * way to drive several GPUs from one process.
 *
 * First use of a handle on a device runs a short self-check of its stepping
 * kernels against its hamEqs kernel (a JIT product does not take the code
 * generator's word for it); HAMK_SELFCHECK=0 skips it.
 */
#ifndef HAMK_H
#define HAMK_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- return codes ------------------------------------------------------ */
#define HAMK_OK               0
#define HAMK_ERR_INVALID     -1   /* bad argument (null pointer, n<=0, ...)  */
#define HAMK_ERR_TAPE        -2   /* malformed tape (forward ref, bad op)    */
#define HAMK_ERR_COMPILE     -3   /* hiprtc specialisation failed            */
#define HAMK_ERR_HIP         -4   /* HIP runtime error                       */
#define HAMK_ERR_NODEVICE    -5   /* no gfx950 device visible                */
#define HAMK_ERR_UNSUPPORTED -6   /* (m,n) outside what the kernels support  */

/* ---- per-trajectory status bits --------------------------------------- */
#define HAMK_ST_SINGULAR   1  /* mass matrix K = J^T M J not invertible (reference: hmatrix `inv` throws) */
#define HAMK_ST_NONFINITE  2  /* state became NaN/Inf                          */
#define HAMK_ST_UNDERFLOW  4  /* adaptive step could not advance time (h -> 0); with gsl_odeiv2 semantics:
                                 GSL_FAILURE out of evolve_apply -- the trajectory stops where it is         */
#define HAMK_ST_MAXSTEPS   8  /* adaptive stepper hit its sub-step budget      */
#define HAMK_ST_DRIFT     16  /* hamk_rk4_steps_checked: the launch lost its energy invariant */

/* ---- where caller pointers live ---------------------------------------- */
#define HAMK_MEM_HOST    0
#define HAMK_MEM_DEVICE  1

/* ---- which space the potential's tape is written in --------------------- */
#define HAMK_U_GENERALIZED 0   /* mkSystem : U(q), n inputs  (Hamilton.hs:201-225) */
#define HAMK_U_CARTESIAN   1   /* mkSystem': U(x), m inputs  (Hamilton.hs:238-254) */

/* ---- expression tape ----------------------------------------------------
 * Op i defines value i; operands a,b are indices of EARLIER values (SSA).
 * The set covers the Num/Fractional/Floating/RealFloat methods a traced
 * Haskell function can emit without comparisons (abs and signum included: they
 * are Num methods; what cannot be recorded is a BRANCH on a value).                            */
enum hamk_opcode {
  HAMK_OP_CONST = 0,  /* c                                  */
  HAMK_OP_INPUT = 1,  /* input[a]                           */
  HAMK_OP_ADD   = 2,  /* v[a] + v[b]                        */
  HAMK_OP_SUB   = 3,  /* v[a] - v[b]                        */
  HAMK_OP_MUL   = 4,  /* v[a] * v[b]                        */
  HAMK_OP_DIV   = 5,  /* v[a] / v[b]                        */
  HAMK_OP_NEG   = 6,  /* -v[a]                              */
  HAMK_OP_RECIP = 7,  /* 1 / v[a]                           */
  HAMK_OP_SIN   = 8,
  HAMK_OP_COS   = 9,
  HAMK_OP_TAN   = 10,
  HAMK_OP_ASIN  = 11,
  HAMK_OP_ACOS  = 12,
  HAMK_OP_ATAN  = 13,
  HAMK_OP_SINH  = 14,
  HAMK_OP_COSH  = 15,
  HAMK_OP_TANH  = 16,
  HAMK_OP_EXP   = 17,
  HAMK_OP_LOG   = 18,
  HAMK_OP_SQRT  = 19,
  HAMK_OP_POWC  = 20, /* v[a] ** c   (constant real exponent; valid for v[a]<0 when c is integral) */
  HAMK_OP_POWI  = 21, /* v[a] ^  b   (b = integer exponent, may be negative)                       */
  HAMK_OP_POW   = 22, /* v[a] ** v[b] (both variable; requires v[a] > 0)                           */
  HAMK_OP_ATAN2 = 23, /* atan2(v[a], v[b])                                                         */
  HAMK_OP_ASINH = 24,
  HAMK_OP_ACOSH = 25,
  HAMK_OP_ATANH = 26,
  HAMK_OP_ABS    = 27, /* |v[a]|     (Num.abs; derivative signum, second derivative 0: not differentiable at 0) */
  HAMK_OP_SIGNUM = 28, /* signum v[a] (Num.signum: -1, 0, +1; derivatives 0)                                   */
  HAMK_OP__COUNT
};

typedef struct hamk_op {
  int32_t op;   /* enum hamk_opcode */
  int32_t a;    /* first operand / input index */
  int32_t b;    /* second operand / integer exponent */
  int32_t _pad;
  double  c;    /* constant (CONST, POWC) */
} hamk_op;

typedef struct hamk_system hamk_system;   /* opaque */

/* ---- options of a system (hamk_system_create_ex) -----------------------------------------------------
 * Everything the library decides for itself when it specialises its kernels for a system can be fixed by the host
 * instead.  HAMK_AUTO (0) in a field leaves that decision to the library.  `size` AND `version` are mandatory: start from
 * hamk_options_init, which sets both and leaves every choice AUTO -- a zero-filled struct with only `size` set (or one built
 * against a header of another layout revision) is refused with HAMK_ERR_INVALID.  The environment variables of DESIGN.md section 7 are TEST
 * overrides: they are read only in a process that sets HAMK_TEST_OVERRIDES=1, and apply only where the field is
 * HAMK_AUTO.  hamk_system_get_options reports what was actually chosen.                                           */
#define HAMK_AUTO 0
#define HAMK_ON   1
#define HAMK_OFF  2
/* which lanes serve one trajectory */
#define HAMK_MAP_LANE 1   /* one trajectory per wavefront lane, everything in registers (n <= 16)                      */
#define HAMK_MAP_WAVE 2   /* wave-cooperative: 16 / 32 / 64 lanes per trajectory, one AD direction per lane, K and its
                             factorisation on the matrix cores and in LDS (any n <= 64; the only mapping for n > 32)   */
#define HAMK_MAP_QUAD 3   /* four lanes per trajectory: every lane runs the sparse per-trajectory AD sweeps, the rows of
                             K are dealt out over the four lanes and factorised in registers with DPP exchanges
                             (17 <= n <= 32 when the coordinate map's Jacobian is sparse, or dense but cheap to evaluate with
                             compile-time seeds -- K is then accumulated in tiles; also usable for n <= 16)              */
/* second-order AD strategy */
#define HAMK_AD_H 1       /* one sweep of full second-order jets                        */
#define HAMK_AD_D 2       /* first-order sweep, then a directional second-order sweep   */
#define HAMK_AD_R 3       /* first-order sweep, then a generated reverse sweep          */
/* stepping-loop bodies */
#define HAMK_BODY_UNROLLED   1
#define HAMK_BODY_STAGE_LOOP 2
/* sincos of the stepping kernels */
#define HAMK_TRIG_DIRECT       1   /* sincos_f64, no table                              */
#define HAMK_TRIG_TABLE        2   /* every evaluation through the 512-pair table in LDS */
#define HAMK_TRIG_TABLE_ROTATE 3   /* one table evaluation per step, stages 2-4 by rotation */
/* which of the two builds of a module its kernels are taken from */
#define HAMK_BUILD_DEFAULT 1
#define HAMK_BUILD_NOLICM  2       /* -mllvm -disable-machine-licm                      */

#define HAMK_OPTIONS_VERSION 0x484b0005u   /* layout revision of hamk_options ('H' 'K' 0x0005: round 5 dropped the dead field
                                              wave_blocked); a struct of another revision is refused with HAMK_ERR_INVALID   */
typedef struct hamk_options {
  uint32_t size;           /* sizeof(hamk_options) as the caller's header has it (hamk_options_init sets it)           */
  uint32_t version;        /* HAMK_OPTIONS_VERSION (hamk_options_init sets it): fields were removed since the first layout,
                              so `size` alone no longer identifies what the caller's header meant                       */
  int32_t mapping;         /* HAMK_MAP_*; AUTO: chosen PER LAUNCH from (n, ensemble size B): a small ensemble of a
                              mid-size system cannot fill the chip with one trajectory per lane.  Two mappings agree to
                              roundoff, not bitwise: pin the mapping where results must not depend on how an ensemble
                              is split into launches (hamk_system_get_options tells what AUTO picks for a size)         */
  int32_t ad_mode;         /* HAMK_AD_*                                                                                 */
  int32_t rk4_body;        /* HAMK_BODY_*                                                                               */
  int32_t rkf_body;        /* HAMK_BODY_*                                                                               */
  int32_t trig;            /* HAMK_TRIG_*                                                                               */
  int32_t gsl_api;         /* 1 | 2 (hamk_system_set_gsl_api); AUTO: 2                                                  */
  int32_t self_check;      /* ON | OFF: first-use self-check of the stepping kernels; AUTO: ON                          */
  int32_t build;           /* HAMK_BUILD_*; AUTO: per kernel, the build that spills fewer SGPRs                         */
  int32_t rk4_min_waves;   /* __launch_bounds__ waves per SIMD of the RK4 kernel; AUTO: measured default                */
  int32_t k_reassoc;       /* ON | OFF: K = J^T M J summed with re-association allowed (repeated Jacobian entries are
                              multiplied by their count instead of added up); AUTO: ON                                  */
  int32_t rk4_park;        /* ON | OFF: lane mapping, RK4 stage loop keeps y and the running combination in LDS across
                              the right-hand side; AUTO: n >= 14                                                        */
  int32_t max_substeps;    /* sub-step budget per stepHam / evolveHam CALL and trajectory (an evolveHam over nt times
                              shares one budget across its intervals; every call of `iterate` has its own); AUTO: 2^24  */
  int32_t cache;           /* ON | OFF: on-disk cache of compiled code objects; AUTO: ON                                */
  int32_t lanes_per_trajectory;  /* OUTPUT of hamk_system_get_options: 1, 4, 16, 32 or 64                               */
  int32_t rkf_park;        /* ON | OFF: QUAD mapping, the adaptive stepper's vectors (y, dydt, k2..k6, trial state) wait in
                              LDS and in a run-time-indexed private array instead of competing with the right-hand side
                              for registers; AUTO: n >= 17.  Lane mapping: follows rkf_body (the stage-loop body IS the
                              parked one since round 4): reported; a value that contradicts rkf_body is refused with
                              HAMK_ERR_UNSUPPORTED when the lane specialisation is built                                 */
  int32_t step_const_vgpr; /* ON | OFF: lane mapping, stepping kernels that rotate sincos pairs: the loop's addend constants (the
                              rotations' Horner addends, the table evaluation's s3 / c4, constant entries of a symbolic 2 x 2 K, grad
                              U's coefficients) are parked in vector registers before the loop; same bits either way; AUTO: ON.  (The
                              slot that used to be padding in front of ensemble_size: 0 = AUTO in every older caller)          */
  int64_t ensemble_size;   /* mapping = AUTO only: the size of the WHOLE ensemble this handle's launches are pieces of (a shard
                              of a multi-GPU run, a chunk of a host loop).  AUTO picks the mapping from the ensemble size, and
                              two mappings agree to roundoff, not bitwise -- so a host that states the whole ensemble's size
                              ONCE (here, or hamk_system_set_ensemble_size) gets every piece computed by the mapping chosen
                              for the whole: any split of the ensemble, over any number of GPUs, reproduces the one-launch
                              bits.  0 (AUTO): every launch stands for itself (mapping from its own B)                     */
  int32_t reserved[12];           /* sizeof(hamk_options) = 128 */
} hamk_options;

/* Zero-fills *opt and sets opt->size.                                                                                 */
void hamk_options_init(hamk_options* opt);

/* ---- system construction (mkSystem / mkSystem') --------------------------
 * inertia[m]; coordinate map f: n inputs -> m outputs f_outs[m] (value ids in
 * f_ops); potential u: scalar output u_out (value id in u_ops) over n
 * (HAMK_U_GENERALIZED) or m (HAMK_U_CARTESIAN) inputs.  Compiles the device
 * module for gfx950; does not need a GPU until the first *_batch call.      */
int hamk_system_create(int32_t m, int32_t n, const double* inertia,
                       const hamk_op* f_ops, int32_t f_nops, const int32_t* f_outs,
                       const hamk_op* u_ops, int32_t u_nops, int32_t u_out,
                       int32_t u_space, hamk_system** out);
/* The same with options (NULL = all defaults = hamk_system_create).  Builds the specialisation the options name; with
 * mapping = HAMK_AUTO the one a large ensemble uses (others are built the first time a launch needs them).            */
int hamk_system_create_ex(int32_t m, int32_t n, const double* inertia,
                          const hamk_op* f_ops, int32_t f_nops, const int32_t* f_outs,
                          const hamk_op* u_ops, int32_t u_nops, int32_t u_out,
                          int32_t u_space, const hamk_options* opt, hamk_system** out);
/* What a launch over B trajectories uses (every field resolved, no HAMK_AUTO left; lanes_per_trajectory filled in).
 * Builds that specialisation if it does not exist yet.                                                                */
int hamk_system_get_options(hamk_system* s, int64_t B, hamk_options* resolved);
/* Makes the introspection entry points below (source, code_size, code_object, build_info, kernel_bytes) describe the
 * specialisation a launch over B trajectories uses (default: the one built at creation).                              */
int hamk_system_describe_batch(hamk_system* s, int64_t B);
/* hamk_options::ensemble_size after creation (0: back to per-launch choice).  A run sharded over G GPUs, or resumed from
 * a checkpoint with another G, calls this with the WHOLE ensemble's size on every handle: results are then independent of
 * the shard layout bit for bit.  No effect where the mapping is fixed by hamk_options::mapping. */
int hamk_system_set_ensemble_size(hamk_system* s, int64_t B_total);
void hamk_system_destroy(hamk_system* s);
int  hamk_system_dims(const hamk_system* s, int32_t* m, int32_t* n);

/* Launch on this HIP stream (hipStream_t as void*; NULL = default stream).  A stream belongs to one device: the
 * binding is made for the device that is CURRENT when this is called and used whenever the handle runs on that
 * device; other devices keep their own (default: the null stream).                                                 */
int hamk_set_stream(hamk_system* s, void* hip_stream);
/* Block until everything queued on the handle's stream of the current device has finished.                         */
int hamk_synchronize(hamk_system* s);

/* Which of the two GSL bindings in hmatrix-gsl's gsl-ode.c stepHam / evolveHam reproduce
 * (`odeSolveV`, Hamilton.hs:445):
 *   2 (default; gsl-ode.c's default build): gsl_odeiv2 -- gsl_odeiv2_driver_apply per output time.
 *     evolve_apply does not write the controller's step size back on a final (clipped) step; the
 *     direction of integration is the sign of the initial step, so a monotone DEcreasing time grid
 *     integrates backwards and a grid that changes direction is HAMK_ERR_INVALID (GSL_EINVAL); a
 *     step that must shrink but cannot is GSL_FAILURE: the trajectory stops, HAMK_ST_UNDERFLOW.
 *   1 (gsl-ode.c built with -DGSLODE1): old gsl_odeiv -- `while (t < ti) gsl_odeiv_evolve_apply`.
 *     h is written back after every accepted step; repeated / decreasing times do no stepping.
 * One trajectory over a single interval (stepHam from h0 = dt/100) takes the same steps under
 * both; they differ from the second output time of evolveHam on, at truncation level (~eps).
 * The environment variable HAMK_GSL_API=1|2 sets the default of new handles.                     */
int     hamk_system_set_gsl_api(hamk_system* s, int32_t api);
int32_t hamk_system_get_gsl_api(const hamk_system* s);

/* Generated HIP source of the specialised module (for inspection/tests).    */
const char* hamk_system_source(const hamk_system* s);
/* Number of bytes of gfx950 code object produced by the specialisation.     */
int64_t hamk_system_code_size(const hamk_system* s);
/* The gfx950 code object(s) the kernels are loaded from (which = 0: default build, 1: the build
 * without MachineLICM, empty unless a kernel is taken from it).  Returns the size in bytes and, if
 * buf != NULL and cap is large enough, copies the ELF into buf -- so a host can disassemble what
 * actually runs (bench.py counts the fp64 instructions of the stepping loop from it).            */
int64_t hamk_system_code_object(const hamk_system* s, int32_t which, void* buf, int64_t cap);
/* One line per kernel: which of the two builds it is taken from (default options, or without
 * MachineLICM when that spills fewer SGPRs), its code bytes and its spilled SGPRs.             */
const char* hamk_system_build_info(const hamk_system* s);
/* Machine-code bytes of one kernel of the module ("hamk_rk4_steps_k", ...); 0 if unknown.
 * kernel_name == NULL: number of function symbols in the module (9 = every device function
 * was inlined into the 8 kernels of the path; the ninth is the self-check's scribble kernel).                                                          */
int64_t hamk_system_kernel_bytes(const hamk_system* s, const char* kernel_name);

/* ---- state functions ------------------------------------------------------ */

/* underlyingPos: x[m][B] = f(q).                          Hamilton.hs:174-178 */
int hamk_coords_batch(hamk_system* s, int64_t B, const double* q, double* x, int32_t mem);

/* toPhase / momenta: p = J^T (M (J qd)).                  Hamilton.hs:262-284 */
int hamk_to_phase_batch(hamk_system* s, int64_t B, const double* q, const double* qd,
                        double* p, int32_t mem);

/* fromPhase / velocities: qd = (J^T M J)^-1 p.            Hamilton.hs:316-337 */
int hamk_from_phase_batch(hamk_system* s, int64_t B, const double* q, const double* p,
                          double* qd, int32_t* status, int32_t mem);

/* Phase-space observables; any output pointer may be NULL.
 * ke = keP (:341-349), pe = pe (:182-186), h = hamiltonian (:353-361).      */
int hamk_observe_batch(hamk_system* s, int64_t B, const double* q, const double* p,
                       double* ke, double* pe, double* h, int32_t* status, int32_t mem);

/* Config-space observables; any output pointer may be NULL.
 * ke = keC (:288-296), lag = lagrangian (:301-309).                          */
int hamk_observe_config_batch(hamk_system* s, int64_t B, const double* q, const double* qd,
                              double* ke, double* lag, int32_t mem);

/* hamEqs: (dq, dp) = (dH/dp, -dH/dq).                     Hamilton.hs:370-387 */
int hamk_hameqs_batch(hamk_system* s, int64_t B, const double* q, const double* p,
                      double* dq, double* dp, int32_t* status, int32_t mem);

/* ---- time stepping ---------------------------------------------------------- */

/* Classic fixed-step RK4 over hamEqs, nsteps steps of dt, IN PLACE on q,p.
 * (BASELINE.json metric: "RK4 phase-space steps/sec".)  status may be NULL.  */
int hamk_rk4_steps(hamk_system* s, int64_t B, double* q, double* p,
                   double dt, int32_t nsteps, int32_t* status, int32_t mem);

/* The same, with the launch checking its own invariant: H = hamiltonian (Hamilton.hs:353-361) is
 * evaluated at entry and exit (two extra evaluations per launch, nothing per step) and
 * HAMK_ST_DRIFT is set where |H_exit - H_entry| > drift_tol * max(1, |H_entry|).  A fixed step
 * through a near-singularity (close encounter of the gravitational systems) is
 * otherwise silently wrong -- the reference's analogous failure raises out of `inv`
 * (Hamilton.hs:321,381).  drift_tol <= 0 disables the check (= hamk_rk4_steps).               */
int hamk_rk4_steps_checked(hamk_system* s, int64_t B, double* q, double* p,
                           double dt, int32_t nsteps, double drift_tol, int32_t* status, int32_t mem);

/* Symplectic fixed-step stepping, IN PLACE on q,p: nsteps steps of dt by the implicit midpoint rule (order = 2) or its
 * three-substep symmetric composition (order = 4); every substep takes `iters` fixed-point iterations (1..64;
 * HAMK_AUTO = 8) -- a fixed count: cost and bits do not depend on convergence.  residual[B] (optional) receives the
 * largest last-iteration update seen; status may be NULL.  One trajectory per lane: n <= 16; HAMK_ERR_UNSUPPORTED
 * for n > 16 or a handle whose options state HAMK_MAP_QUAD / HAMK_MAP_WAVE.  No reference counterpart.
 *   One substep of size h from y = [q; p]: z = y; `iters` times z <- y + (h/2) hamEqs(z); then y <- 2 z - y.  order = 4 takes
 *   substeps g1 dt, g2 dt, g1 dt with g1 = 1 / (2 - 2^(1/3)), g2 = 1 - 2 g1.  dt < 0 steps back (the method is time-reversible).
 *   residual = max over steps, substeps and components j of |z_j(last) - z_j(last but one)| / max(1, |y_j|): how a caller
 *   learns that `iters` was too small for its dt; no status bit says so.  status: HAMK_ST_SINGULAR from any right-hand side,
 *   HAMK_ST_NONFINITE where the final state is not finite.
 *   Mapping: a handle with mapping = HAMK_AUTO ALWAYS runs this stepper on its one-trajectory-per-lane module, whatever B is
 *   (for RK4, AUTO may pick HAMK_MAP_QUAD for small ensembles of mid-size systems; that rule does not apply here).
 *   HAMK_MEM_DEVICE: asynchronous on the handle's stream; HAMK_MEM_HOST: staged, returns with the results in place.
 *   B == 0 or nsteps == 0: HAMK_OK, nothing launched -- and nothing written: q, p, residual and status are left as they are
 *   (a caller that reads residual / status after such a call clears them first).  The kernel lives in a companion module of the lane module, built the
 *   first time one of these three entry points asks for it; the first-use self-check does not cover it.                  */
int hamk_symplectic_steps(hamk_system* s, int64_t B, double* q, double* p, double dt, int32_t nsteps,
                          int32_t order, int32_t iters, double* residual, int32_t* status, int32_t mem);
/* Source / one build_info-format line (kernel, bytes, spilled SGPRs and VGPRs) of the companion module; builds it if
 * needed; needs no GPU.  NULL + hamk_last_error() where the stepper is unsupported for this handle.               */
const char* hamk_symplectic_source(hamk_system* s);
const char* hamk_symplectic_build_info(hamk_system* s);

/* Largest-Lyapunov-exponent stepping fused with classic RK4 (Benettin's two-trajectory method), IN PLACE on q, p, wq, wp and
 * logsum.  Per trajectory: the state y = [q; p], a deviation vector w = [wq; wp] (arrays shaped like q, p) and a running
 * logsum[B].  One interval: s = y + d0 w; `every` times y <- RK4(y, dt) and s <- RK4(s, dt); then delta = s - y,
 * d = sqrt(sum_j delta_j^2) over all 2n components, logsum += log(d / d0), w = delta / d.  A call runs `nintervals` intervals in
 * one launch; the estimate of the largest Lyapunov exponent is logsum / (nintervals every dt), the caller's division.
 *   w is used EXACTLY AS GIVEN, not normalised at entry: a unit vector (Euclidean norm over all 2n components) is the caller's
 *   business, and a w of norm c adds log c to the first term of logsum.  logsum is read, added to and written back.  So a run cut
 *   into calls, w and logsum carried over, reproduces the bits of the one call.  q, p do not depend on w or d0: they are what the
 *   same RK4 steps alone give.
 *   q, p, wq, wp, logsum are required; status may be NULL.  status: HAMK_ST_SINGULAR from any right-hand side of either
 *   trajectory, HAMK_ST_NONFINITE where the final state, w or logsum is not finite (d = 0 gives log 0 and is flagged this way).
 *   HAMK_ERR_INVALID: a null handle or required array, B < 0, nintervals < 0, every < 1, nintervals * every beyond int32, dt not
 *   finite, d0 not finite or <= 0, an unknown mem.  One trajectory per lane: n <= 16; HAMK_ERR_UNSUPPORTED for n > 16 or a handle
 *   whose options state HAMK_MAP_QUAD / HAMK_MAP_WAVE; mapping = HAMK_AUTO ALWAYS runs on the one-trajectory-per-lane module,
 *   whatever B is.  HAMK_MEM_DEVICE: asynchronous on the handle's stream; HAMK_MEM_HOST: staged, returns with the results in place.
 *   B == 0 or nintervals == 0: HAMK_OK, nothing launched and nothing written.  The kernel (hamk_lyap.hpp) lives in a companion
 *   module of the lane module, built the first time one of these three entry points asks for it; the first-use self-check does
 *   not cover it.  No reference counterpart.                                                                              */
int hamk_lyapunov_steps(hamk_system* s, int64_t B, double* q, double* p, double* wq, double* wp, double dt,
                        int32_t nintervals, int32_t every, double d0, double* logsum, int32_t* status, int32_t mem);
/* Source / one build_info-format line (kernel, bytes, spilled SGPRs and VGPRs, allocated VGPRs, function symbols) of that
 * companion module; builds it if needed; needs no GPU.  NULL + hamk_last_error() where the stepper is unsupported.     */
const char* hamk_lyapunov_source(hamk_system* s);
const char* hamk_lyapunov_build_info(hamk_system* s);

/* Poincare sections fused with classic RK4: `nsteps` RK4 steps of dt IN PLACE on q, p (the right-hand side and the step of
 * hamk_lyapunov_steps, one trajectory per lane), and after every step the crossing of ONE component of y = [q; p] through a
 * surface, located inside the step and recorded inside the launch.
 *   The surface.  coord in [0, 2n): yc = q[coord] for coord < n, p[coord - n] otherwise.  period == 0: the plane yc = level.
 *   period > 0: the family yc = level (mod period) -- angles need it: a pendulum that flips over winds its angle past 2 pi.
 *   The cell index c(y) = floor((yc - level) / period) for period > 0, (yc >= level ? 0 : -1) for period == 0, a double.
 *   A step from y0 to y1 crosses UPWARD where c(y1) > c(y0), the target value being level + c(y1) period, and DOWNWARD where
 *   c(y1) < c(y0), target level + c(y0) period.  direction: +1 counts upward crossings only, -1 downward only, 0 both; "upward" is
 *   in stepping order, whatever the sign of dt.  AT MOST ONE crossing is recorded per step: dt is expected to resolve the motion
 *   (a step that passes several members of the family, or leaves and re-enters a cell, records one crossing or none).  A step
 *   with a non-finite yc at either end (a NaN compares false) records nothing.
 *   Where inside the step: theta in [0, 1] with Yc(theta) = target on RK4's own third-order continuous extension
 *       Y(theta) = y0 + dt [b1 k1 + b2 (k2 + k3) + b4 k4],  b1 = theta - 3 theta^2 / 2 + 2 theta^3 / 3,  b2 = theta^2 - 2 theta^3 / 3,
 *       b4 = -theta^2 / 2 + 2 theta^3 / 3   (Y(1) is the RK4 step; no extra right-hand side, nothing carried between steps),
 *   from the secant value (target - y0c) / (y1c - y0c) by FOUR Newton iterations, theta clamped to [0, 1] after each, a non-finite
 *   update leaving theta as it was.  The hit is Y(theta) in all 2n components; the section component is stored as computed, not
 *   snapped to the target.
 *   Outputs.  qhit, phit: [max_hits][n][B]; thit: [max_hits][B], may be NULL; nhit: [B].  nhit is READ, ADDED TO AND WRITTEN BACK:
 *   a crossing goes to row nhit[i] if that row exists (0 <= nhit[i] < max_hits) and is counted either way, so nhit > max_hits is how
 *   a caller learns of an overflow; rows at or beyond the count are never written.  thit = (double)(step0 + step index) + theta, in
 *   units of dt, step0 being the caller's count of steps already taken.  So N steps in one call equal N1 + N2 in two calls with
 *   step0 = N1 and the buffers carried over, bit for bit on every output; and q, p do not depend on the surface arguments.
 *   q, p, qhit, phit, nhit are required; thit and status may be NULL.  status: HAMK_ST_SINGULAR from any right-hand side,
 *   HAMK_ST_NONFINITE where the final state is not finite.
 *   HAMK_ERR_INVALID: a null handle or required array, B < 0, nsteps < 0, coord outside [0, 2n), dt or level not finite, period
 *   negative or not finite, direction outside {-1, 0, 1}, max_hits < 1, max_hits * n * B beyond 2^48 elements, step0 < 0 or beyond
 *   2^52, an unknown mem.  One trajectory per lane: n <= 16; HAMK_ERR_UNSUPPORTED for n > 16 or a handle whose options state
 *   HAMK_MAP_QUAD / HAMK_MAP_WAVE; mapping = HAMK_AUTO ALWAYS runs on the one-trajectory-per-lane module, whatever B is.
 *   HAMK_MEM_DEVICE: asynchronous on the handle's stream; HAMK_MEM_HOST: staged (the hit buffers and nhit both ways), returns with
 *   the results in place.  B == 0 or nsteps == 0: HAMK_OK, nothing launched and nothing written.  The kernel (hamk_psec.hpp) lives
 *   in a companion module of the lane module, built the first time one of these three entry points asks for it; the first-use
 *   self-check does not cover it.  No reference counterpart.                                                              */
int hamk_poincare_steps(hamk_system* s, int64_t B, double* q, double* p, double dt, int32_t nsteps, int32_t coord, double level,
                        double period, int32_t direction, int32_t max_hits, double* qhit, double* phit, double* thit,
                        int32_t* nhit, int64_t step0, int32_t* status, int32_t mem);
/* Source / one build_info-format line (kernel, bytes, spilled SGPRs and VGPRs, allocated VGPRs, function symbols) of that
 * companion module; builds it if needed; needs no GPU.  NULL + hamk_last_error() where the stepper is unsupported.     */
const char* hamk_poincare_source(hamk_system* s);
const char* hamk_poincare_build_info(hamk_system* s);

/* First-exit times fused with classic RK4: up to `nsteps` RK4 steps of dt IN PLACE on q, p (the right-hand side and the step of
 * the Poincare-section stepper, one trajectory per lane), and after every step the test whether the trajectory has left a region; a trajectory
 * that has left STOPS, and a wavefront whose trajectories have all stopped ends its stepping: finished work is dropped.
 *   The region.  1 .. HAMK_EXIT_MAX_GATES gates in HOST memory (whatever mem says), each a component of y = [q; p] -- coord in
 *   [0, 2n): q[coord] for coord < n, p[coord - n] otherwise -- and a closed interval [lo, hi], lo < hi, either bound may be
 *   infinite; `reserved` is ignored.
 *   Per-trajectory state, READ, UPDATED AND WRITTEN BACK.  code[B]: HAMK_EXIT_ALIVE (-1) still running; 2 g + side >= 0 stopped by
 *   gate g through its lower (side 0) or upper (side 1) bound; HAMK_EXIT_NONFINITE (-2) stopped because the state stopped being
 *   finite.  texit[B], in units of dt.  qexit, pexit [n][B]: the state at the exit; both NULL or both given.  A trajectory is
 *   alive iff its code at entry is exactly -1 (a new run: every code -1); any other value counts as stopped, and of a trajectory
 *   stopped at entry nothing is read but its code and nothing is written but status (0): q, p, code, texit, qexit, pexit keep
 *   their bits.
 *   A step of an alive trajectory from y0 to y1.  Any component of y1 not finite: code -2, texit = step0 + step index + 1,
 *   HAMK_ST_NONFINITE, qexit / pexit untouched.  Otherwise gate g FIRES where its component at y1 lies outside [lo, hi]; the target
 *   is the violated bound, and theta in [0, 1] with Yc(theta) = target is located on RK4's third-order continuous extension from the
 *   secant value by FOUR Newton iterations, theta clamped to [0, 1] after each, a non-finite update leaving theta as it was (see
 *   the Poincare-section stepper above).  A component already outside at y0 -- an alive trajectory's first step only -- has theta = 0.  The firing
 *   gate with the smallest theta wins, on a tie the lowest index: code = 2 g + side, texit = (double)(step0 + step index) + theta,
 *   step0 being the caller's count of steps already taken; qexit, pexit receive Y(theta) in all 2n components, the gate component
 *   as computed, not snapped to the bound.  Either way q, p become y1, the END of the exit step, and are not advanced again.
 *   So: N steps in one call equal N1 + N2 in two calls with step0 = N1 and the arrays carried over, bit for bit on every output;
 *   a stopped trajectory's q, p are those of a call with nsteps = floor(texit) - step0 + 1 (floor(texit) - step0 for code -2);
 *   while a trajectory is alive its q, p do not depend on the gates, nor on any other trajectory.
 *   q, p, gates, code, texit are required; status may be NULL.  status: HAMK_ST_SINGULAR from any right-hand side of a step the
 *   trajectory was alive in, HAMK_ST_NONFINITE with code -2.
 *   HAMK_ERR_INVALID: a null handle or required array, exactly one of qexit / pexit, B < 0, nsteps < 0, ngates outside
 *   1 .. HAMK_EXIT_MAX_GATES, a coord outside [0, 2n), a NaN bound or lo >= hi, dt not finite, step0 < 0 or beyond 2^52, an unknown
 *   mem.  One trajectory per lane: n <= 16; HAMK_ERR_UNSUPPORTED for n > 16 or a handle whose options state HAMK_MAP_QUAD /
 *   HAMK_MAP_WAVE; mapping = HAMK_AUTO ALWAYS runs on the one-trajectory-per-lane module, whatever B is.
 *   HAMK_MEM_DEVICE: asynchronous on the handle's stream; HAMK_MEM_HOST: staged (code, texit, qexit, pexit both ways), returns with
 *   the results in place.  B == 0 or nsteps == 0: HAMK_OK, nothing launched and nothing written.  The kernel (hamk_exit.hpp) lives
 *   in a companion module of the lane module, built the first time one of these three entry points asks for it; the first-use
 *   self-check does not cover it.  No reference counterpart.                                                              */
#define HAMK_EXIT_MAX_GATES 4
#define HAMK_EXIT_ALIVE     -1
#define HAMK_EXIT_NONFINITE -2
typedef struct hamk_gate {
  int32_t coord;
  int32_t reserved;
  double lo, hi;
} hamk_gate;
int hamk_exit_steps(hamk_system* s, int64_t B, double* q, double* p, double dt, int32_t nsteps, const hamk_gate* gates,
                    int32_t ngates, int32_t* code, double* texit, double* qexit, double* pexit, int64_t step0, int32_t* status,
                    int32_t mem);
/* Source / one build_info-format line (kernel, bytes, spilled SGPRs and VGPRs, allocated VGPRs, function symbols) of that
 * companion module; builds it if needed; needs no GPU.  NULL + hamk_last_error() where the stepper is unsupported.     */
const char* hamk_exit_source(hamk_system* s);
const char* hamk_exit_build_info(hamk_system* s);

/* Trajectory recording fused with classic RK4: `nsteps` RK4 steps of dt IN PLACE on q, p (the right-hand side and the step of the
 * Lyapunov stepper, one trajectory per lane), and on a grid of steps the state and / or its Hamiltonian written to fixed-size row
 * buffers from inside the launch: evolveHam's rows (Hamilton.hs:433-462, row 0 the initial state) on a fixed step.
 *   Rows.  G is the number of steps taken in the whole run: step0 (the caller's count of steps already taken) at entry,
 *   step0 + s + 1 after the call's step s.  Where G is a multiple of `every`, the state after G steps is row k = G / every.  Row 0
 *   is recorded at entry and only if step0 == 0: the state as given, bit for bit.  A row is recorded after every step whose G in
 *   (step0, step0 + nsteps] is a multiple of `every`.  A row k >= max_rows is dropped; rows outside this call's range are never
 *   written, and no row is ever read.  After the call min(max_rows, (step0 + nsteps) / every + 1) rows of the run are filled.
 *   Outputs.  qout, pout: [max_rows][n][B], both NULL or both given; row k is an [n][B] block in this header's layout, so every
 *   *_batch entry point applies to it as it stands.  hout: [max_rows][B], may be NULL: the Hamiltonian of the recorded state
 *   (hamk_observe_batch's h; evaluated only where a row is recorded).  At least one of the two groups must be given; hout alone is
 *   the energy curve of an ensemble at 1 / (4n) of the memory.
 *   So: N steps in one call equal N1 + N2 in two calls with step0 = N1 and the buffers carried over, bit for bit on q, p and every
 *   row; the final q, p do not depend on every, max_rows or on which outputs are given.  The rows are this stepper's bits; they are
 *   not promised equal to hamk_rk4_steps's.
 *   status may be NULL.  status: HAMK_ST_SINGULAR from any right-hand side and from the Hamiltonian's solve, HAMK_ST_NONFINITE where
 *   the final state is not finite; a non-finite trajectory's rows hold what the arithmetic gives.
 *   HAMK_ERR_INVALID: a null handle, q or p, exactly one of qout / pout, all three outputs NULL, B < 0, nsteps < 0, every < 1,
 *   max_rows < 1, max_rows n B beyond 2^48, step0 < 0 or beyond 2^52, dt not finite, an unknown mem.  One trajectory per lane:
 *   n <= 16; HAMK_ERR_UNSUPPORTED for n > 16 or a handle whose options state HAMK_MAP_QUAD / HAMK_MAP_WAVE; mapping = HAMK_AUTO
 *   ALWAYS runs on the one-trajectory-per-lane module, whatever B is.
 *   HAMK_MEM_DEVICE: asynchronous on the handle's stream.  HAMK_MEM_HOST: staged; exactly the rows this call fills are copied back,
 *   every other row of the caller's buffers keeps its bits, and the buffers are not copied in.  B == 0 or nsteps == 0: HAMK_OK,
 *   nothing launched and nothing written, row 0 included.  The kernel (hamk_rec.hpp) lives in a companion module of the lane
 *   module, built the first time one of these three entry points asks for it; the first-use self-check does not cover it.     */
int hamk_record_steps(hamk_system* s, int64_t B, double* q, double* p, double dt, int32_t nsteps, int32_t every, int32_t max_rows,
                      double* qout, double* pout, double* hout, int64_t step0, int32_t* status, int32_t mem);
/* Source / one build_info-format line (kernel, bytes, spilled SGPRs and VGPRs, allocated VGPRs, function symbols) of that
 * companion module; builds it if needed; needs no GPU.  NULL + hamk_last_error() where the stepper is unsupported.     */
const char* hamk_record_source(hamk_system* s);
const char* hamk_record_build_info(hamk_system* s);

/* stepHam dt: adaptive RKF45 with GSL's standard controller from 0 to dt,
 * h0 = dt/100, eps_abs = eps_rel = 1.49012e-08, IN PLACE.  Hamilton.hs:390-402,
 * :445-448.  nsub (optional, [B]) receives accepted+rejected sub-step counts. */
int hamk_step_ham_batch(hamk_system* s, int64_t B, double* q, double* p, double dt,
                        int32_t* status, int32_t* nsub, int32_t mem);

/* `iterate (stepHam dt)` (README.md:150; the demo's frame loop, app/Examples.hs:429): ncalls consecutive
 * stepHam dt in ONE launch, IN PLACE.  Every call is what a separate hamk_step_ham_batch would do -- a fresh
 * evolveHam over (0, dt): t = 0, h0 = dt/100 (Hamilton.hs:400-402, :447), its own sub-step budget -- and the
 * result is bit-identical to ncalls separate calls BY CONSTRUCTION on every mapping (every call starts with the
 * instructions a separate launch starts with, its own evaluation of dydt_in included); what is saved is
 * ncalls - 1 launches and stream synchronisations (one trajectory is launch-latency bound: BASELINE config 1).
 * out_every > 0: the state after every out_every-th call goes to qout/pout, [ncalls / out_every][n][B]
 * (the frames an animation shows); out_every == 0: qout/pout may be NULL.  status: OR over the calls;
 * nsub: sub-steps summed over the calls.                                                                 */
int hamk_step_ham_iterate(hamk_system* s, int64_t B, double* q, double* p, double dt, int32_t ncalls,
                          int32_t out_every, double* qout, double* pout,
                          int32_t* status, int32_t* nsub, int32_t mem);

/* evolveHam: states at each of the nt >= 2 requested times ts[] (host array);
 * qout/pout are [nt][n][B]; row 0 is the initial state (Hamilton.hs:443-462).
 * h0 = (ts[1]-ts[0])/100 and the step size carries across output times, as in
 * hmatrix-gsl's `odeSolveV` (how exactly: hamk_system_set_gsl_api).  Pass h0 <= 0 /
 * eps <= 0 for the reference defaults.                                         */
int hamk_evolve_ham_batch(hamk_system* s, int64_t B, const double* q0, const double* p0,
                          int32_t nt, const double* ts, double* qout, double* pout,
                          double h0, double eps_abs, double eps_rel,
                          int32_t* status, int32_t* nsub, int32_t mem);

/* ---- initial conditions of an ensemble, generated on the device ------------------------------------
 * q[j][i], qd[j][i] of trajectories first_index .. first_index + B - 1: uniform in [q_lo[j], q_hi[j]] and
 * [qd_lo[j], qd_hi[j]] (host arrays of n entries), from a counter-based generator keyed by (seed, GLOBAL
 * trajectory index, field) -- splitmix64, hamk_sample.hpp -- so a rank of a sharded run fills its own shard in
 * HBM without a host array or a scatter, and every shard layout draws bit-identical inputs.
 * Same bits as the Python sampler the CPU tests use (hamilton_amd/examples.py sample_config).  The reference has no
 * counterpart: its demo starts one trajectory from a command-line Config (app/Examples.hs:230-359).                */
int hamk_sample_batch(hamk_system* s, int64_t B, int64_t first_index, uint64_t seed,
                      const double* q_lo, const double* q_hi, const double* qd_lo, const double* qd_hi,
                      double* q, double* qd, int32_t mem);

/* ---- devices and device memory ---------------------------------------------
 * For hosts that do not link HIP themselves (the Haskell shim, plain C): with these an ensemble
 * can live in HBM across calls (HAMK_MEM_DEVICE) and one process can drive every GPU of a node --
 * one handle per device, the calling thread's current device selects where a handle runs.  The
 * reference has no counterpart (it is a single-trajectory CPU library); they exist because the
 * north_star's "state resident in HBM" and "shard over 8 GPUs, gather at the end" must be reachable
 * through the C ABI alone.                                                                      */
int hamk_set_device(int32_t device);                 /* current device of the calling thread      */
int hamk_get_device(int32_t* device);
int hamk_device_malloc(void** ptr, int64_t bytes);   /* on the current device                     */
int hamk_device_free(void* ptr);
#define HAMK_COPY_H2D 0
#define HAMK_COPY_D2H 1
#define HAMK_COPY_D2D 2   /* same or another device (peer copy over xGMI)                        */
int hamk_memcpy(void* dst, const void* src, int64_t bytes, int32_t kind);   /* synchronous        */
/* Final gather of a sharded ensemble: part g is a structure-of-arrays block [n][B_parts[g]] in
 * device memory (any device); out is [n][sum_g B_parts[g]], trajectories in part order -- in host
 * memory (out_mem = HAMK_MEM_HOST) or on the current device (HAMK_MEM_DEVICE; peer copies over
 * xGMI).  One array per call (q, then p).  Synchronous; it does not wait for launches still
 * running on other streams -- hamk_synchronize the handles that produce the parts first.        */
int hamk_gather_batch(int32_t nparts, int32_t n, const int64_t* B_parts, const double* const* parts,
                      double* out, int32_t out_mem);

/* The same final gather for hosts that run ONE PROCESS PER GPU ("RCCL over xGMI only for
 * the final gather"; the reference has no counterpart): a process has no peer pointers to hand to
 * hamk_gather_batch, it needs a communicator.  Rank 0 draws an id (HAMK_COMM_ID_BYTES opaque bytes) and ships
 * it to the other processes by whatever host channel the launcher offers (a file, a socket, MPI_Bcast); every
 * process selects its device (hamk_set_device) and calls hamk_comm_create with the same id and world and its
 * own rank -- collectively: the call returns when all ranks have arrived.  hamk_comm_allgather_batch is
 * collective too: part is this rank's structure-of-arrays block [n][B_parts[rank]] on the communicator's
 * device, out [n][sum_g B_parts[g]] on the same device, trajectories in rank order on EVERY rank; B_parts
 * (host array, world entries) must be the same on all ranks.  Equal shards take one ncclAllGather per row,
 * ragged ones one ncclBroadcast per (rank, row), fused in one RCCL group either way.  One array per call (q,
 * then p).  Runs on the NULL stream and returns when the data is there; hamk_synchronize the handle that
 * produced part first.  RCCL is loaded on first use: a box without librccl gets HAMK_ERR_UNSUPPORTED from
 * these four calls and loses nothing else.                                                                     */
#define HAMK_COMM_ID_BYTES 128
typedef struct hamk_comm hamk_comm;
int hamk_comm_unique_id(void* id);                                        /* HAMK_COMM_ID_BYTES bytes out   */
int hamk_comm_create(const void* id, int32_t world, int32_t rank, hamk_comm** out);
int hamk_comm_allgather_batch(hamk_comm* comm, int32_t n, const int64_t* B_parts, const double* part,
                              double* out);
int hamk_comm_destroy(hamk_comm* comm);                                   /* NULL is fine                   */

/* ---- ensemble checkpoint (no reference counterpart) -----------------------
 * One file = 64-byte header (magic "HAMKCKP1", n, B, steps_done, seed, t), q[n][B], p[n][B] as raw
 * little-endian fp64, SHA-256 of all of it.  q, p may be host or device arrays (mem); device state
 * is staged in 8 MiB pieces.  Written aside and renamed: a crash leaves the previous file.
 * steps_done / seed / t are the caller's bookkeeping (per-index splitmix64 seed of the initial
 * conditions, steps taken, model time) and come back from hamk_checkpoint_info.  Every kernel is a
 * pure function of the state, so a resumed run continues bit-identically -- on the same mapping: a run
 * resumed with a different shard layout states the whole ensemble's size (hamk_system_set_ensemble_size)
 * or pins hamk_options::mapping, as the original run must have.
 * Device state is copied on the NULL stream: hamk_synchronize the handle (or synchronise the stream that
 * produced / will consume q, p) before a write and before using the arrays after a read.  A header that does
 * not match the file's size is rejected before anything is allocated from it.                      */
int hamk_checkpoint_write(const char* path, int32_t n, int64_t B, const double* q, const double* p,
                          int32_t mem, int64_t steps_done, uint64_t seed, double t);
int hamk_checkpoint_info(const char* path, int32_t* n, int64_t* B, int64_t* steps_done,
                         uint64_t* seed, double* t);                    /* outputs may be NULL */
int hamk_checkpoint_read(const char* path, int32_t n, int64_t B, double* q, double* p, int32_t mem);

/* ---- diagnostics ---------------------------------------------------------- */
const char* hamk_last_error(void);
const char* hamk_version(void);
/* Number of visible HIP devices (0 if none / runtime missing).               */
int hamk_device_count(void);

#ifdef __cplusplus
}
#endif
#endif /* HAMK_H */
