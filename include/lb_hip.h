/*
 * lb_hip.h -- C ABI of liblbhip.so, the MI355X (gfx950) D2Q9 lattice-Boltzmann engine.
 *
 * This is the drop-in boundary for the collide-and-stream path of
 * latticeboltzmann/2d-lb.  In the reference that path sits behind pyopencl:
 * `cl.Program(...).build()` gives `self.kernels`, every step method is
 * `self.kernels.<name>(queue, global, local, *buffers, scalars).wait()` and all
 * state lives in `cl.Buffer`s (LB_D2Q9/dimensionless/opencl_dim.py:203-255,
 * 295-370, 390-415, 495-518).  Each entry point below names the reference
 * interface it replaces.
 *
 * Conventions
 *  - plain pointers and sizes only; no C++ or torch types cross this boundary.
 *  - every function returns 0 on success or a negative lb_status; the message
 *    of the last failure on the calling thread is lb_last_error().
 *  - host arrays are borrowed for the duration of the call.  Field layout on
 *    the host is the reference's device layout: plane-major, x fastest,
 *    idx(k,x,y) = k*nx*H + y*nx + x (== the F-ordered (nx,ny[,9]) numpy arrays
 *    of opencl_dim.py:165,279,390-415), H = rows of the slab this handle owns.
 *  - work is enqueued asynchronously on the handle's HIP stream; lb_sync() and
 *    every lb_get_* wait for it (the reference waits after every kernel).
 *  - one host thread per handle.
 */
#ifndef LB_HIP_H
#define LB_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LB_ABI_VERSION 11

typedef enum {
    LB_OK = 0,
    LB_ERR_ARG = -1,      /* bad argument / unsupported combination           */
    LB_ERR_HIP = -2,      /* a HIP runtime call failed (no device, OOM, ...)  */
    LB_ERR_STATE = -3,    /* call not valid in the handle's current state     */
    LB_ERR_COMM = -4      /* RCCL failure                                     */
} lb_status;

/* Boundary-condition families.  PIPE is the reference's `move_bcs`
 * (D2Q9.cl:173-261); PERIODIC and CAVITY are build-defined (BASELINE configs
 * 2-4) and specified by oracle/d2q9_oracle.c; VELOCITY_INLET is the reference's
 * second rule set of D2Q9.cl. */
typedef enum {
    LB_BC_PIPE = 0,       /* pressure inlet x=0 / outlet x=nx-1, no-slip y=0,ny-1 */
    LB_BC_PERIODIC = 1,   /* periodic in x and y                               */
    LB_BC_CAVITY = 2,     /* four no-slip walls, north wall moving with lid_u  */
    LB_BC_VELOCITY_INLET = 3, /* D2Q9.cl:263-374: imposed speed inlet_u at x=0 / outlet_u at x=nx-1, north and
                             south rows copy their missing links from the opposite wall row.  Dead code in
                             the reference's `dimensionless` package (only OLD/opencl.py:281-327 launches
                             it).  Whole-grid handles; lb_run fuses it (up to four time steps per launch; from
                             three on the wall-row bands are advanced as a small lattice of their own), the phase
                             entry points run it un-fused. */
    LB_BC_OPEN = 4,       /* scalar lattices (LB_SEM_DIFFUSION) only: the box of the reference's Diffusion classes, whose move_bcs
                             is `pass` (reaction_diffusion/diffusion.py): a link that would enter from outside the box keeps the
                             value it had when the populations were last set -- the handle's edge state (lb_get_edge_state). */
    LB_BC_BOX = 5,        /* coupled scalar lattices (LB_SEM_MULTIFIELD) only: the closed box of the reference's
                             D2Q9_multifield_fisher.cl, whose move_bcs bounces every link that would enter from outside back on
                             the node itself (f1 := f3 at x = 0, ...), on all four walls.  Two links per corner are neither
                             streamed nor bounced: the handle's corner state (lb_get_corner_state). */
    LB_BC_DIRICHLET = 6,  /* the LB Poisson solver (LB_SEM_POISSON) only: the box of the reference's D2Q9_poisson.cl, whose move_bcs
                             prescribes a value on all four walls: on each wall and in each corner the three links pointing into the
                             box become w_k R, R = -(sum of the cell's five other non-rest links + (w0 - 1) rho_on_boundary) /
                             (sum of the three weights).  Two links per corner are neither streamed nor written, and the corner's
                             rule reads them: the handle's corner state, LB_BC_BOX's eight links in the same order. */
    LB_BC_ZERO_GRADIENT = 7 /* forced flow in a porous medium (LB_SEM_POROUS) only: the open box of the reference's
                             porous_media/single_component.cl, whose move_open_bcs gives every boundary cell all nine post-stream
                             populations of the interior cell (clamp(x, 1, nx-2), clamp(y, 1, ny-2)).  Every link the push `move`
                             leaves stale at the boundary is overwritten: no edge or corner state.  nx, ny >= 3. */
} lb_bc_mode;

/* Which of the reference's two (numerically different) paths the handle reproduces.
 * OPENCL: LB_D2Q9/D2Q9.cl driven as opencl_dim.py:372-387 does -- the fused, fast path.
 * CYTHON: LB_D2Q9/dimensionless/cython_dim.pyx:160-359 -- boundary rules before streaming, bounce-back
 *         walls, restricted in-place streaming, moment overrides; PIPE family, whole-grid handles
 *         (a compatibility path for users of the reference's CPU classes: lb_run launches the boundary
 *         phase + one fused pass per step, the phase entry points one kernel each).
 * OPENCL_D2Q9I: see below. */
typedef enum {
    LB_SEM_OPENCL = 0,
    LB_SEM_CYTHON = 1,
    LB_SEM_OPENCL_D2Q9I = 2,  /* LB_D2Q9/D2Q9i.cl driven as dimensionless/opencl_dim_D2Q9i.py does: the "incompressible"
                                 fork of the OpenCL path -- momentum in place of velocity (D2Q9i.cl:90-94), inner =
                                 rho + 3 cu + 4.5 cu^2 - 1.5 usq (:58), re-derived inlet / outlet (:194-205), u, v
                                 re-zeroed in the obstacle every step.  PIPE family, whole-grid handles; fused like the
                                 OpenCL path.  Restated as the fork has it: it is unstable (tests/golden/o2_d2q9i_53x27). */
    LB_SEM_DIFFUSION = 3,     /* a SCALAR lattice: LB_D2Q9/D2Q9_diffusion.cl driven as reaction_diffusion/diffusion.py does -- a
                                 concentration rho carried by D2Q9 populations with the linear equilibrium feq_k = w_k rho (1 + 3 c_k.u),
                                 an IMPOSED velocity field u, v (lb_set_macro, lb_set_velocity_from; no kernel writes it) and an optional
                                 Fisher growth term w_k G rho (1 - rho) (lb_set_reaction).  Families LB_BC_PERIODIC (build-defined)
                                 and LB_BC_OPEN (the reference's box); whole-grid GPU handles.  lb_run fuses the reference's five
                                 launches per step into one (k_ad_step: 72 B of populations + 8 B of u, v per cell and step) or,
                                 bitwise equal, four steps into one launch through LDS tiles (k_ad_tile4): n = 4a + r steps run
                                 as a tile launches, then r single steps.  lb_set_variant: 0 = k_ad_step only; bit 9 = the
                                 tiles, on any box, with bits 2-3 = 0 the tile shape by size, 1 / 2 / 3 = 32 x 16 cells two per
                                 thread / 32 x 16 one / 16 x 16; -1 (default) = the tiles on boxes of 256^2 ... 8192^2 cells,
                                 where they measured 2.0-3.0 x k_ad_step's rate (8192^2: 162-192 k against 69-71 k MLUPS, the
                                 latter 0.89-0.91 of the copy rate on the same handle: profiles/scalar_bench.txt).  A run
                                 always stores rho in its last launch -- with G != 0 rho is not a moment of what a run leaves
                                 behind.  omega, nx, ny are the only other lb_params fields it reads. */
    LB_SEM_MULTIFIELD = 4,    /* ONE FIELD of a set of coupled scalar lattices: LB_D2Q9/D2Q9_multifield_fisher.cl driven as
                                 advecting_range_expansion/deterministic_fisher_waves.py does.  A scalar lattice in every respect
                                 above (whole-grid GPU handle, imposed u, v, lb_set_reaction = this field's G, rho always stored),
                                 except that the growth term of field i is w_k G_i rho_i (1 - sum_j rho_j) over the fields
                                 advanced together (lb_run_coupled; lb_run = the set of one), and that the families are
                                 LB_BC_PERIODIC (build-defined) and LB_BC_BOX (the reference's closed box).  One fused launch
                                 per time step for the whole set (k_mf_step: 72 B of populations per field + 8 B of u, v per
                                 cell and step); lb_set_variant takes -1 and 0 only (no LDS tiles for coupled sets). */
    LB_SEM_POISSON = 5,       /* the LB POISSON SOLVER: LB_D2Q9/D2Q9_poisson.cl driven as poisson/solver.py does -- a D2Q9 relaxation
                                 whose fixed point solves a Poisson problem in a box: rho = (9/5)(f1 + ... + f8), feq_0 = (w0 - 1) rho,
                                 feq_k = w_k rho, f_k (1 - omega) + omega feq_k + w_k source react_factor, a prescribed value on the four
                                 walls (LB_BC_DIRICHLET, the only family), and a run loop that stops when rho has stopped changing.
                                 Whole-grid GPU handles without obstacles; omega, nx, ny are the only lb_params fields read
                                 (lb_set_poisson has the rest).  One fused launch per iteration (k_ps_step: 88 B per cell) that
                                 also leaves the two sums of the reference's convergence test, one small launch that folds them and
                                 sets a device-side stop word (k_ps_check), no host wait but one 4-byte read-back per batch of
                                 iterations: lb_solve, below.  u, v of such a handle are written by lb_gradient only.
                                 lb_set_variant takes -1 and 0 only. */
    LB_SEM_POROUS = 7,        /* (6 is not assigned: the suite holds lb_create to refusing semantics 6 in a periodic box as unknown,
                                 tests/test_poisson_cpu.py.)  FORCED FLOW IN A POROUS MEDIUM: LB_D2Q9/porous_media/single_component.cl driven as
                                 single_component.py's Simulation_Runner.run does with one fluid -- a D2Q9 BGK fluid with Guo forcing,
                                 a porosity epsilon in the equilibrium and in the forcing term, a linear drag (nu_fluid / K), a
                                 quadratic one (Fe / sqrt(K)) and constant or position-dependent body forces; families
                                 LB_BC_PERIODIC and LB_BC_ZERO_GRADIENT.  Whole-grid GPU handles without obstacles; omega, nx, ny
                                 are the only lb_params fields read (lb_set_porous, lb_set_body_force, lb_set_force_field have
                                 the rest).  lb_run: one fused launch per step (k_pm_step: 72 B per cell, 80 B with a force
                                 field; the last launch of a run also stores rho, u, v, the total force and the barycentric
                                 velocity, + 28 B).  float32 like every lattice here (the reference's fork computes in
                                 float64).  lb_set_variant takes -1 and 0 only. */
    LB_SEM_MULTIFLUID = 9,    /* (8 is not assigned either: tests/test_porous_cpu.py holds lb_create to refusing semantics 8 in a
                                 periodic box as unknown.)  MULTICOMPONENT SHAN-CHEN FLUIDS: LB_D2Q9/multicomponent_multiphase/multi.cl
                                 driven as multi.py's Simulation_Runner.run does -- 1 ... 3 D2Q9 BGK fluids on one grid, one handle
                                 each, relaxing towards an equilibrium at the barycentric velocity of all of them, with Guo forcing by
                                 body forces and by pseudopotential interaction forces (a D2Q9 stencil over a function of the
                                 neighbours' density: the step is not local to the cell), and with mass-exchange reactions; families
                                 LB_BC_PERIODIC and LB_BC_ZERO_GRADIENT, nx, ny >= 3.  Whole-grid GPU handles without obstacles;
                                 omega, nx, ny are the only lb_params fields read.  lb_run_fluids advances a set (below). */
    LB_SEM_ROCKET = 11        /* (10 is not assigned either: tests/test_multifluid_cpu.py holds lb_create to refusing semantics 10 in a
                                 periodic box as unknown.)  SURFACTANT-PROPELLED COLONIES: LB_D2Q9/rocket_yeast/rocket_yeast.cl and
                                 rocket_yeast_forces_only.cl driven as rocket_yeast.py's Rocket_Yeast.run does -- ONE LATTICE of a set
                                 of exactly two scalar lattices on one periodic grid, the growing population and the surfactant it
                                 secretes; the velocity that advects both is a D2Q9 stencil over the surfactant (a Marangoni flow)
                                 and the population feels a Shan-Chen self-attraction (a second stencil): the step is not local to
                                 the cell.  A scalar lattice in every respect above (whole-grid GPU handle, linear equilibrium, rho
                                 always stored, lb_check), except that no call imposes its velocity; family LB_BC_PERIODIC only,
                                 nx, ny >= 3.  omega, nx, ny are the only lb_params fields read (lb_set_rocket has the rest).
                                 lb_run_rocket advances a set (below). */
} lb_semantics;

typedef struct {
    int32_t nx, ny;           /* global grid (reference: self.nx, self.ny, opencl_dim.py:191-201) */
    int32_t y0, local_ny;     /* row slab [y0, y0+local_ny) owned by this handle; 0, ny for one GPU */
    int32_t bc_mode;          /* lb_bc_mode */
    int32_t device;           /* HIP device ordinal, or LB_DEVICE_CPU */
    float omega;              /* np.float32(self.omega), opencl_dim.py:369 */
    float inlet_rho;          /* np.float32(self.inlet_rho), :336 */
    float outlet_rho;
    float lid_u;              /* CAVITY only */
    float rho0;               /* CAVITY corner closure density */
    int32_t flags;            /* LB_FLAG_* */
    int32_t semantics;        /* lb_semantics; 0 = the OpenCL path */
    float inlet_u, outlet_u;  /* VELOCITY_INLET only: u_w, u_e of OLD/opencl.py:283-286 */
    int32_t reserved[1];      /* must be zero */
} lb_params;

/* lb_params.device = LB_DEVICE_CPU: the product's own CPU backend (2d-lb_amd/csrc/cpu_backend.h): the reference's CPU class
 * LB_D2Q9/dimensionless/cython_dim.pyx Pipe_Flow.run (:346-359) restated for the host, single-threaded like the reference, in
 * the reference's mixed float32 / float64 arithmetic.  Needs semantics = LB_SEM_CYTHON, bc_mode = LB_BC_PIPE, a whole-grid
 * handle and no flags.  BASELINE.json's first configuration ("256 x 256 Poiseuille, CPU path, no GPU") runs on it without a
 * GPU in the box, and bench.py times it next to the GPU numbers.  It is selected by this value and by nothing else: a handle
 * with a device ordinal >= 0 never falls back to the host.  Entry points that only make sense on a device (lb_set_stream,
 * the slab / halo / comm / peer calls, lb_run_group, lb_run_batch, lb_autotune*, lb_copy_calibration, the corner state) return
 * LB_ERR_STATE on such a handle; u, v are float64 inside, float32 across the ABI like everywhere else. */
#define LB_DEVICE_CPU (-1)

/* (declared below: lb_set_params_f64 hands a CPU-backend handle the reference's float64 omega / inlet_rho / outlet_rho, which
 *  lb_params carries as float32) */

/* Treat the handle as a row slab with ghost rows even when it owns the whole grid: its halo
 * is then filled by lb_halo_import / the RCCL exchange (a 1-rank periodic ring sends to
 * itself).  Lets the multi-GPU code path run, and be tested, on a single GPU. */
#define LB_FLAG_HALO 1
/* Device layout of the two lattices.  Default: the nine plane-rows of a lattice row are stored together
 * ([row][plane][pitch]); with this flag each plane is contiguous ([plane][row][pitch], the round-1 layout).  Results are
 * bit-identical; the marching kernels stream ~12 % faster from interleaved rows at 8192^2. */
#define LB_FLAG_PLANAR 2
/* rho, u, v after lb_run.  BGK relaxation conserves rho and rho*u, so the moments of the post-collision populations a run
 * leaves behind are the rho, u, v of its last step (the reference stores the pre-collision moments, opencl_dim.py:384-385:
 * equal up to rounding).  By default lb_run therefore stores nothing but the populations in the PIPE / PERIODIC / CAVITY
 * families of the OpenCL path, and the fields are rebuilt from them by one device pass the first time they are asked for
 * (lb_get_macro, lb_update_feq, ..., or before anything else overwrites the populations).  With this flag the last launch
 * of every lb_run stores them itself, as round 2 did (12 B per cell more in that launch).  The other families /
 * semantics always store: their fields are not plain moments (imposed inlet speeds, wall overrides, momentum). */
#define LB_FLAG_EAGER_MACRO 4

/* Obstacle-mask rows a slab keeps of each neighbour (lb_set_mask_halo): the fourteen-step halo cycle (two
 * seven-step launches per exchange, ABI 8) recomputes seven of the neighbour's rows and reads the mask six rows
 * beyond them.  (ABI 7: 9 rows, the ten-step cycle.) */
#define LB_MASK_HALO_ROWS 13

typedef struct lb_sim lb_sim; /* opaque: device buffers, streams, events, RCCL communicator */

/* ---- lifetime (replaces init_opencl + allocate_constants + the cl.Buffer
 *      allocations of __init__, opencl_dim.py:165-176, 203-255) ------------- */
int lb_abi_version(void);
int lb_device_count(void);                     /* <0 on error */
const char *lb_last_error(void);
int lb_create(const lb_params *p, lb_sim **out);
int lb_destroy(lb_sim *s);
/* CPU backend only (LB_DEVICE_CPU): the reference keeps omega, inlet_rho and outlet_rho as np.float64 and its mixed-precision
 * expressions see them as such (cython_dim.pyx:86-95, 139-141); lb_params rounds them to float32.  This call restores the
 * float64 values, which makes the backend reproduce the reference's populations bit for bit.  LB_ERR_STATE on a GPU handle
 * (the device kernels compute in float32 throughout). */
int lb_set_params_f64(lb_sim *s, double omega, double inlet_rho, double outlet_rho);
int lb_sync(lb_sim *s);
/* Run everything on an externally owned hipStream_t (e.g. a stream the caller
 * made with hipStreamCreate, or torch.cuda.Stream().cuda_stream) instead of the
 * handle's own; pass NULL to go back.  Waits for the work enqueued on the stream
 * it leaves.  NULL always means the handle's own stream (hipStreamNonBlocking:
 * ordered with no other stream), so the legacy default stream -- whose handle is
 * NULL, and which is torch's current stream unless the caller made another one
 * current -- cannot be named: a caller whose other work runs there moves it to a
 * stream of its own and passes that one, or orders the two with events. */
int lb_set_stream(lb_sim *s, void *hip_stream);

/* ---- host <-> device state (replaces cl.Buffer(COPY_HOST_PTR, hostbuf=...)
 *      and cl.enqueue_copy, opencl_dim.py:291-293, 323-327, 395-407, 502) ---- */
int lb_set_macro(lb_sim *s, const float *rho, const float *u, const float *v);  /* each [H][nx]   */
int lb_get_macro(lb_sim *s, float *rho, float *u, float *v);
int lb_set_f(lb_sim *s, const float *f);       /* [9][H][nx]; also fills f_streamed (:323-327) */
int lb_get_f(lb_sim *s, float *f);
int lb_get_feq(lb_sim *s, float *feq);         /* [9][H][nx] */
int lb_set_mask(lb_sim *s, const int32_t *mask); /* [H][nx], 1 = solid (opencl_dim.py:468, 502); NULL clears */
/* VELOCITY_INLET only: the eight corner links that no kernel of that rule set ever writes (the reference's push
 * `move` drops what would enter from outside the box, D2Q9.cl:151-169, and the rules skip them): they keep the
 * values f had at the last lb_set_f / lb_init_pop -- in the reference inside its f_streamed buffer.  Order:
 * f1(0,0), f8(0,0), f1(0,ny-1), f5(0,ny-1), f3(nx-1,0), f7(nx-1,0), f3(nx-1,ny-1), f6(nx-1,ny-1).  A checkpoint
 * needs them next to f (lb_set_f resets them).
 * LB_SEM_MULTIFIELD handles (LB_BC_BOX): likewise the eight corner links the push `move` of D2Q9_multifield_fisher.cl never
 * writes and its move_bcs skips, in this order:
 * f6(0,0), f8(0,0), f5(nx-1,0), f7(nx-1,0), f5(0,ny-1), f7(0,ny-1), f6(nx-1,ny-1), f8(nx-1,ny-1)
 * (eight zeros that nothing reads in the PERIODIC family). */
int lb_get_corner_state(lb_sim *s, float *out8);
int lb_set_corner_state(lb_sim *s, const float *in8);

/* ---- scalar lattices (LB_SEM_DIFFUSION; LB_ERR_STATE on every other handle) ------------------------------------------
 * lb_set_reaction: G of collide_particles_fisher (D2Q9_diffusion.cl:95-124), in lattice units; 0 (the default) = plain
 * collide_particles.
 * Edge state (LB_BC_OPEN; zero floats in the PERIODIC family): the links that enter a cell from outside the box.  The
 * reference's push `move` never writes them and copy_buffer restores them from f_streamed, so they hold, whenever a step
 * reads them, the values they had at the last lb_set_f / lb_init_pop -- which capture them; a checkpoint needs them beside f.
 * lb_edge_floats() = 6 (nx + ny) floats, in this order:
 *   west column x = 0:     f1[ny], f5[ny], f8[ny]      east column x = nx-1:  f3[ny], f6[ny], f7[ny]
 *   south row y = 0:       f2[nx], f5[nx], f6[nx]      north row y = ny-1:    f4[nx], f7[nx], f8[nx]
 * Four corner links appear twice (f5(0,0), f8(0,ny-1), f6(nx-1,0), f7(nx-1,ny-1)): the column's entry is the one the
 * kernels read, lb_get_edge_state returns the same value in both places.
 * lb_set_velocity_from: u, v of `flow` (any GPU flow handle of the same nx x ny that owns its whole grid, on the same
 * device) become the scalar handle's imposed velocity, device to device, after the flow handle's lazily rebuilt fields
 * were brought up to date; ordered behind the flow handle's enqueued work, never waits on the host. */
int lb_set_reaction(lb_sim *s, float G);
int lb_edge_floats(lb_sim *s);
int lb_get_edge_state(lb_sim *s, float *out);
int lb_set_edge_state(lb_sim *s, const float *in);
int lb_set_velocity_from(lb_sim *s, lb_sim *flow);

/* ---- the noisy collision of a scalar lattice (LB_SEM_DIFFUSION only: LB_ERR_STATE on a field of a coupled set, the Poisson
 *      solver and every other kind) -- collide_particles_noisy_fisher, D2Q9_diffusion.cl:127-167, as reaction_diffusion/
 *      noisy_fisher_wave.py drives it:  react = G rho (1 - rho) + sqrt(Dg rho (1 - rho)) z,  f_k = relaxed f_k + w_k react,
 *      f_k < 0 -> 0 (a compare: rho outside [0, 1] makes all nine links NaN, as in the reference; lb_check counts such cells).
 * z is a standard normal per cell and collision from a counter-based stream, drawn in registers inside the kernels: Philox4x32-10,
 * key = the low and high word of `seed`, counter = (x / 4, y, t_lo, t_hi) for the four cells x = 4j .. 4j+3 of row y, t = the noise
 * counter: the number of noisy collisions since the seed was set.  Word r -> u = float(r >> 9) 2^-23 + 2^-24; cells 0, 1 of the
 * four get R cos(theta), R sin(theta), R = sqrt(-2 ln u(r0)), theta = 2 pi u(r1); cells 2, 3 the same from r2, r3.  The same
 * bits in every kernel form, however a run is split, and after a checkpoint.  Not pyopencl's generator (the reference draws unseeded).
 * lb_set_noise: Dg > 0 switches the handle to the noisy cell and sets t = 0; Dg == 0 switches back to the plain cell; a
 *   negative or non-finite Dg: LB_ERR_ARG.  lb_run, lb_run_screened and lb_collide_particles honour it, one count of t per collision.
 * lb_get_noise / lb_set_noise_counter: for checkpoints (any of Dg, seed, t may be NULL).
 * lb_noise_fill: the [ny][nx] normals of noise counter t under the handle's seed, by the device function the kernels inline;
 *   on_device != 0: out is a device pointer.  Waits for the handle's work.
 * lb_set_noise_field: a supplied [ny][nx] field (on_device != 0: a device pointer; copied) that lb_collide_particles uses in
 *   place of the stream -- the reference's random_normal buffer; NULL drops it.  While one is set lb_run returns LB_ERR_STATE
 *   (the reference's run never uses a field twice).  Not part of a checkpoint. */
int lb_set_noise(lb_sim *s, float Dg, uint64_t seed);
int lb_get_noise(lb_sim *s, float *Dg, uint64_t *seed, uint64_t *t);
int lb_set_noise_counter(lb_sim *s, uint64_t t);
int lb_noise_fill(lb_sim *s, uint64_t t, float *out, int on_device);
int lb_set_noise_field(lb_sim *s, const float *z, int on_device);

/* ---- the LB Poisson solver (LB_SEM_POISSON; LB_ERR_STATE on every other handle) --------------------------------------
 * A fresh handle is the reference's start: f = 0, rho = 0, source = 0, corner state = 0, iteration counter = 0.
 * lb_set_poisson: rho_on_boundary, the value prescribed on the walls (default 0); react_factor, the `delta_t * D` of the
 *   reference's collide_particles (default 1): every cell adds w_k source react_factor.  (The reference's class scales the
 *   source by lb_D delta_t once more on the host, update_source: the caller's business, LB_D2Q9.poisson does it.)
 *   tolerance, of lb_solve's stopping rule (default 1e-6).
 * lb_set_source / lb_get_source: the source field, [ny][nx] floats.  on_device != 0: src is a device pointer to that dense
 *   layout and the copy into the handle's padded plane never goes through the host (ordered on the handle's stream; the
 *   caller has finished writing src).
 * lb_solve: up to max_iterations iterations of solver.py's run loop.  After every iteration whose index n (counted since
 *   the last lb_solve_reset; lb_run's iterations count as well) is >= 2 the device forms
 *   ratio = mean |rho - rho_before| / mean rho_before (sums in a fixed order: reproducible) and, if ratio < tolerance --
 *   false for the inf and NaN of a lattice that starts at zero --, sets its stop word to n.  Launches are enqueued in batches
 *   with no host wait inside a batch; the launches of a batch behind the stop do nothing, so what the call leaves is exactly
 *   the state after n iterations: the reference's.  *iterations_done = iterations made by this call, *converged = 1 if it
 *   stopped by the rule, *last_ratio = the ratio of the last iteration checked (NaN: none yet).  Any may be NULL.  Waits for
 *   the handle's work.  The counter persists between calls (solver.py's num_iterations); a call after a stop goes on.
 * lb_solve_reset: the counter back to 0 (what update_source does); rho and the populations stay.
 * lb_get_solve_state / lb_set_solve_state: the counter and the stop word (0, or the iteration a solve stopped at), for
 *   checkpoints.
 * lb_gradient: central differences of rho over 2 dx, inv_two_dx = 1 / (2 dx), 0 for a neighbour outside the box:
 *   ddx[y nx + x] = (rho(x+1, y) - rho(x-1, y)) inv_two_dx, ddy likewise in y.  One launch writes them into the handle's u and
 *   v fields (lb_get_macro returns them from then on: nothing else ever writes u, v of such a handle), then each is copied
 *   to nx ny floats at ddx / ddy: device pointers, or host pointers (hipMemcpyDefault), or NULL for no copy.  Waits for the
 *   handle's work.  (The reference's update_negative_gradient stores MINUS the y-difference in `u` and MINUS the x-difference
 *   in `v`; LB_D2Q9.poisson.Poisson_Solver keeps that.)
 * On such a handle lb_run(n) = n fused iterations with no check and no early out (the last stores rho), lb_move ...
 * lb_collide_particles, lb_init_pop are the reference's phases, lb_get_corner_state / lb_set_corner_state work as on
 * LB_BC_BOX; lb_set_reaction, lb_set_velocity_from, lb_check, lb_autotune* and every slab / mask call: LB_ERR_STATE. */
int lb_set_poisson(lb_sim *s, float rho_on_boundary, float react_factor, float tolerance);
int lb_set_source(lb_sim *s, const float *src, int on_device);
int lb_get_source(lb_sim *s, float *src);
int lb_solve(lb_sim *s, int max_iterations, int *iterations_done, int *converged, float *last_ratio);
int lb_solve_reset(lb_sim *s);
int lb_get_solve_state(lb_sim *s, int *iterations, int *stop_word);
int lb_set_solve_state(lb_sim *s, int iterations, int stop_word);
int lb_gradient(lb_sim *s, float inv_two_dx, float *ddx, float *ddy);

/* ---- forced flow in a porous medium (LB_SEM_POROUS; LB_ERR_STATE on every other handle) ------------------------------------
 * One time step, every stage after the first two local to the cell (single_component.py:679-751):
 *   1. move_periodic / move + copy_streamed_onto_f                               lb_move
 *   2. move_open_bcs (LB_BC_ZERO_GRADIENT only)                                  lb_move_bcs
 *   3. update_hydro_pourous: rho = sum f, u, v = sum f c / rho if rho > 1e-6, else 0   lb_update_hydro
 *   4. G := the constant body force [+ the force field]                          }
 *   5. update_forces_pourous: if rho > 1e-6, G := epsilon G - epsilon nu_fluid u / K   } lb_update_forces
 *      - epsilon Fe |u| u / sqrt(K) with the u, v of stage 3; else G := 0        }
 *   6. update_bary_velocity: u_b = (sum f c + rho G / 2) / rho                    lb_update_bary_velocity
 *      (rho = 0 gives NaN, as in the reference: not guarded)
 *   7. update_feq_pourous: feq_k = w_k rho (1 + 3 c.u_b + 4.5 (c.u_b)^2 / epsilon - 1.5 u_b^2 / epsilon)      lb_update_feq
 *   8. collide_particles_pourous: f_k (1 - omega) + omega feq_k
 *      + w_k rho (1 - omega / 2)(3 c.G + 9 (c.G)(c.u_b) / epsilon - 3 u_b.G / epsilon)   lb_collide_particles
 * lb_run(n) = n fused steps; bitwise equal to the eight stages called one by one.  rho, u, v (lb_get_macro), the total force
 * (lb_get_force) and u_b (lb_get_bary_velocity) are those of the last step, before its collision.
 * lb_set_porous: epsilon, nu_fluid, K, Fe (defaults 1, 0, 1, 0); LB_ERR_ARG for epsilon <= 0, K <= 0 or a non-finite value.
 * lb_set_body_force: the sum of the constant forces (default 0, 0).
 * lb_set_force_field: two [ny][nx] planes added to the constant force in every cell (the reference's add_radial_body_force
 *   depends on position only); on_device != 0: device pointers to that dense layout, copied device to device on the handle's
 *   stream (the caller has finished writing them, or wrote them on that stream; the call returns with the copy complete).
 *   gx = gy = NULL drops the field.
 * lb_get_force / lb_get_bary_velocity / lb_set_bary_velocity: [ny][nx] planes; an output may be NULL.
 * lb_set_f, lb_get_f, lb_get_feq, lb_set_macro, lb_get_macro, lb_init_pop, lb_hot_kernel, lb_plan_launches and lb_layout
 * work as on every handle.  Masks, slabs and halo calls, lb_autotune*, lb_set_variant with a value other than -1 and 0,
 * lb_run_batch, lb_run_coupled, lb_solve*, lb_set_reaction, lb_set_velocity_from, lb_check and the edge / corner state:
 * LB_ERR_STATE. */
int lb_set_porous(lb_sim *s, float epsilon, float nu_fluid, float K, float Fe);
int lb_set_body_force(lb_sim *s, float gx, float gy);
int lb_set_force_field(lb_sim *s, const float *gx, const float *gy, int on_device);
int lb_get_force(lb_sim *s, float *Gx, float *Gy);
int lb_set_force(lb_sim *s, const float *Gx, const float *Gy);     /* (checkpoints: what lb_get_force returned) */
int lb_set_bary_velocity(lb_sim *s, const float *u_bary, const float *v_bary);
int lb_get_bary_velocity(lb_sim *s, float *u_bary, float *v_bary);
int lb_update_forces(lb_sim *s);            /* stages 4 and 5 */
int lb_update_bary_velocity(lb_sim *s);     /* stage 6 */

/* ---- multicomponent Shan-Chen fluids (LB_SEM_MULTIFLUID; LB_ERR_STATE on every other handle) --------------------------------
 * A SET is 1 ... 3 handles of one geometry, family, layout flag and device, advanced together; fluid i of a table is the i-th
 * handle of the array a call is given.  One time step (multi.py:729-803):
 *   1. per fluid: move_periodic / move + copy_streamed_onto_f, then move_open_bcs (LB_BC_ZERO_GRADIENT)     lb_move, lb_move_bcs
 *   2. per fluid: update_hydro_fluid: rho = sum f; u, v = sum f c / rho if rho > 1e-12, else 0              lb_update_hydro
 *      (u, v are stored and never read by the dynamics)
 *   3. G_i := (g_i [+ the force field]) rho_i, then for every entry of the interaction table, in order,     lb_update_forces_fluids
 *      with S_j(x) = sum_k w_k c_k psi(rho_j(x + c_k)): G_i -= G_int psi(rho_i) S_j, G_j -= G_int psi(rho_j) S_i.
 *      The neighbour is the wrapped cell (LB_BC_PERIODIC) or the cell clamped to [0, n-1] (LB_BC_ZERO_GRADIENT).
 *      G is a FORCE here (a force per density on a porous handle).  fluid_1 == fluid_2: both increments land on
 *      the one fluid, a self-interaction acts with 2 G_int, as in the reference.
 *   4. u_b = sum_i (sum_k f_ik c_k + G_i / 2) / sum_i rho_i (NaN where the total density is 0: not guarded)  lb_update_bary_fluids
 *   5. per fluid: feq_k = w_k rho_i (1 + 3 c.u_b + 4.5 (c.u_b)^2 - 1.5 u_b^2)                                 lb_update_feq
 *   6. per fluid: f_k (1 - omega_i) + omega_i feq_k + (1 - omega_i / 2) w_k (3 c.G_i + 9 (c.G_i)(c.u_b) - 3 u_b.G_i)   lb_collide_particles
 *   7. the reaction table, in order, on the rho of stage 2:                                                  lb_react_fluids
 *      LB_REACT_EAT   phi = (a - b) / (a + b); growth = rate a b where |phi| < cutoff, else 0; f_eater,k += w_k growth, f_eatee,k -= w_k growth
 *      LB_REACT_GROW  f_k += w_k rate where min < rho < max
 * lb_run_fluids(n) = n steps on one stream without a host wait, of ONE launch each (k_mc_step: a workgroup puts rho_i of its rows
 * and their halo into LDS and runs stages 3-7 in registers) or of two (lb_set_variant(0): k_mc_moments stores every rho_i, k_mc_collide
 * gathers again and reads rho around the cell); both bitwise equal to the stages called one by one.
 * lb_run on such a handle is the set of one; so are lb_update_forces and lb_update_bary_velocity.  The tables are stored with the
 * set's FIRST handle and read from there by every set call.  rho, u, v (lb_get_macro), G (lb_get_force) and u_b
 * (lb_get_bary_velocity, the same on every member) are those of the last step, before its collision.
 * lb_set_body_force: this fluid's acceleration g; lb_set_force_field: a position-dependent acceleration added to it; both are
 * multiplied by rho in the kernel.  lb_get_force / lb_set_force / lb_set_bary_velocity / lb_get_bary_velocity as on a porous handle.
 * lb_set_interactions: n <= 6 entries; potential LB_PSI_LINEAR (psi = rho), LB_PSI_SHAN_CHEN (psi = rho_0 (1 - exp(-rho / rho_0)),
 *   parameter = rho_0 != 0), LB_PSI_POW (psi = rho^alpha, parameter = alpha); rho < 0 counts as 0.  boundary = the stencil's rule:
 *   0 periodic, 1 zero gradient -- it must be the set's family (LB_ERR_ARG otherwise).  n = 0 clears the table.
 * lb_set_reactions: n <= 4 entries; an eater must differ from its eatee.
 * lb_set_variant on the set's first handle: -1 (the planner's choice: the one-launch step at every size, profiles/multifluid_bench.txt), 0 (the two-launch step),
 *   1 (the one-launch step k_mc_step: a workgroup owns six rows -- three fluids: two -- of a 256-cell tile, puts rho_i of them, of
 *   one halo row above and below and one halo cell left and right into LDS, and runs stages 3-7 after one barrier; bitwise the
 *   same result).  lb_hot_kernel and lb_steps_per_launch report what runs.
 * Masks, slabs and halo calls, lb_autotune*, lb_run_group / batch / coupled, lb_solve*, lb_set_reaction, lb_set_velocity_from,
 * lb_check, the edge / corner state and lb_set_porous: LB_ERR_STATE naming LB_SEM_MULTIFLUID. */
enum { LB_PSI_LINEAR = 0, LB_PSI_SHAN_CHEN = 1, LB_PSI_POW = 2 };
enum { LB_REACT_EAT = 0, LB_REACT_GROW = 1 };
typedef struct {
    int32_t fluid_1, fluid_2;   /* indices into the set */
    int32_t potential;          /* LB_PSI_* */
    int32_t boundary;           /* 0 periodic, 1 zero gradient: the set's family */
    float G_int, parameter;
} lb_interaction;
typedef struct {
    int32_t kind;               /* LB_REACT_* */
    int32_t fluid_a, fluid_b;   /* eat: eater, eatee; grow: the fluid, unused */
    float p0, p1, p2;           /* eat: rate, cutoff, unused; grow: min, max, rate */
} lb_fluid_reaction;
int lb_run_fluids(lb_sim **fluids, int count, int n_steps);
int lb_set_interactions(lb_sim **fluids, int count, const lb_interaction *table, int n);
int lb_set_reactions(lb_sim **fluids, int count, const lb_fluid_reaction *table, int n);
int lb_get_interactions(lb_sim *first, lb_interaction *table, int *n);      /* table: room for 6; either may be NULL */
int lb_get_reactions(lb_sim *first, lb_fluid_reaction *table, int *n);      /* table: room for 4 */
int lb_update_forces_fluids(lb_sim **fluids, int count);    /* stage 3 */
int lb_update_bary_fluids(lb_sim **fluids, int count);      /* stage 4 */
int lb_react_fluids(lb_sim **fluids, int count);            /* stage 7 */

/* ---- surfactant-propelled colonies (LB_SEM_ROCKET; LB_ERR_ARG, with the reason, for a count other than 2, a handle given twice,
 *      a handle of another semantics or members of different geometry, layout or device) ---------------------------------------
 * A SET is exactly two handles of one geometry, layout flag and device: fields[0] the population p, fields[1] the surfactant c,
 * each with its own omega.  With grad_w a (x) = sum_k w_k c_k a(x + c_k), the D2Q9 stencil with periodic wrap, and
 * 1 / cs^2 = float32(1. / (cs cs)) of cs = float32(1 / sqrt(3)), one time step (rocket_yeast.py:469-483) is
 *   1. both lattices stream periodically (move_periodic, then the copy back)                                  lb_move
 *   2. rho_i = sum_k f_ik, k = 0 ... 8                                                                         lb_update_hydro
 *   3. LB_ROCKET_FLOW (the class Rocket_Yeast):                                                                lb_update_velocity_rocket,
 *        (u, v) = -epsilon (1 / cs^2) grad_w rho_c                                                             lb_update_forces_rocket
 *        psi = rho_o (1 - exp(-max(rho_p, 0) / rho_o));  F = -G_chen psi(x) grad_w psi
 *      LB_ROCKET_FORCES (the class Rocket_Yeast_Forces_Only; forces first, then the velocity):
 *        S = pow(1 - exp(-max(rho_c, 0) / c_o), alpha);  F_s = -epsilon (1 / cs^2) grad_w S
 *        F_p = -G_chen (1 / cs^2) grad_w rho_p (rho_p - rho_o);  (u, v) = F_p + F_s
 *   4. feq_ik = w_k rho_i (1 + 3 c_k.u) for both lattices                                                      lb_update_feq
 *   5. population: max(0, f_k (1 - omega) + omega feq_k + w_k G rho_p (1 - rho_p) [FLOW: + w_k (c_k.F) / cs^2]);  lb_collide_rocket
 *      FORCES: no growth where rho_p > 1.  Surfactant: f_k (1 - omega_c) + omega_c feq_k + w_k G_c rho_p.
 * lb_run_rocket(n) = n steps on one stream without a host wait, of ONE launch each (k_ry_step: a workgroup puts the two stencil
 * operands of its ten rows of a 256-cell tile and of their halo into LDS and runs stages 3-5 on populations kept in registers) or of
 * two (lb_set_variant(0) on the set's first handle: k_ry_moments stores both densities, k_ry_collide gathers again and reads them
 * around the cell); both bitwise equal to the stages called one by one.  lb_set_variant takes -1 (the planner's choice), 0 and 1;
 * lb_hot_kernel, lb_steps_per_launch and lb_plan_launches report what runs.
 * The parameters are stored with the set's FIRST handle.  A run leaves f after the last collision, and rho (lb_get_macro: the
 * member's own), u, v (lb_get_macro on either member: the set's), psi / S and the forces (lb_get_rocket_fields) of the last step,
 * before its collision; they are stored by the run's last launch only.
 * lb_run, lb_run_coupled / batch / fluids / group, masks, slab and halo calls, lb_autotune*, lb_solve*, lb_set_reaction,
 * lb_set_velocity_from, lb_set_porous, the interaction and reaction tables, the edge and corner state and lb_collide_particles:
 * LB_ERR_STATE naming LB_SEM_ROCKET. */
enum { LB_ROCKET_FLOW = 0, LB_ROCKET_FORCES = 1 };
typedef struct {
    int32_t mode;               /* LB_ROCKET_* */
    float G, G_c;               /* the population's growth rate and the surfactant's secretion rate, in lattice units */
    float epsilon;              /* the velocity's coupling to the surfactant */
    float rho_o, G_chen;        /* the self-attraction: saturation density (FLOW: != 0) and strength */
    float c_o, alpha;           /* FORCES: the surfactant concentration at which the surface saturates (!= 0), its exponent */
} lb_rocket_params;
int lb_set_rocket(lb_sim **fields, int count, const lb_rocket_params *params);
int lb_get_rocket(lb_sim *first, lb_rocket_params *params);
int lb_run_rocket(lb_sim **fields, int count, int n_steps);
int lb_update_velocity_rocket(lb_sim **fields, int count);   /* stage 3: u, v (FORCES: from the stored forces) */
int lb_update_forces_rocket(lb_sim **fields, int count);     /* stage 3: psi and F / S, F_s and F_p */
int lb_collide_rocket(lb_sim **fields, int count);           /* stage 5 */
/* [ny][nx] each, any may be NULL: psi (FLOW) or S (FORCES); the pseudo-force F (FLOW) or the pressure force F_p (FORCES); the
 * surface force F_s (FORCES; zeros in FLOW) */
int lb_get_rocket_fields(lb_sim **fields, int count, float *psi_or_S, float *Fx, float *Fy, float *Fsx, float *Fsy);

/* ---- the reference's per-phase methods, one kernel each (slow, un-fused;
 *      API and test parity).  Single-slab handles only. ------------------- */
int lb_move(lb_sim *s);                 /* kernels.move + kernels.copy_buffer, opencl_dim.py:339-353 */
int lb_move_bcs(lb_sim *s);             /* kernels.move_bcs (+ bounceback_in_obstacle), :329-337, 510-518 */
int lb_update_hydro(lb_sim *s);         /* kernels.update_hydro, :355-362 */
int lb_update_feq(lb_sim *s);           /* kernels.update_feq, :295-306 */
int lb_collide_particles(lb_sim *s);    /* kernels.collide_particles, :364-370 */
int lb_zero_velocity_in_obstacle(lb_sim *s); /* kernels.set_zero_velocity_in_obstacle, :506-508 */
int lb_init_pop(lb_sim *s);             /* f = f_streamed = feq (device side of init_pop, :308-327) */

/* ---- the hot path: n time steps (replaces the body of Pipe_Flow.run, opencl_dim.py:372-387:
 *      move -> move_bcs(+obstacle) -> update_hydro -> update_feq -> collide_particles, 6-8 launches and
 *      as many host waits per step) by fused launches that advance one to four time steps each
 *      (k_step, k_step2, k_step3, k_step4, k_tile4; results bitwise independent of which) and no host wait.
 *      rho,u,v are those of the LAST step: rebuilt on demand from the populations it left in the plain
 *      families (see LB_FLAG_EAGER_MACRO), stored by the last launch in the others; feq is rebuilt from them on
 *      demand.  Handles with LB_SEM_CYTHON run the first step's boundary phase as a launch of its own, then one
 *      pass per step (k1_fstep) or per four steps (k1_tile4, LDS tiles), each pass ending with the next step's
 *      boundary rule.
 *      Multi-slab handles exchange their halo rows inside lb_run when a communicator is attached
 *      (lb_comm_init), otherwise the caller drives lb_step_boundary / lb_halo_export /
 *      lb_halo_import / lb_step_interior. */
int lb_run(lb_sim *s, int n_steps);

/* ---- row-slab decomposition (new: the reference is single-device) -------- */
/* One fused step split in two launches so the halo exchange can overlap the
 * interior: boundary = local rows {0, H-1}, interior = rows 1..H-2.
 * lb_step_finish swaps the lattices.  write_macro != 0 also stores rho,u,v. */
int lb_step_boundary(lb_sim *s, int write_macro);
int lb_step_interior(lb_sim *s, int write_macro);
int lb_step_finish(lb_sim *s);
/* Halo rows of the lattice that the NEXT step will read (= the one being written between
 * lb_step_boundary and lb_step_finish, the current one otherwise).  side 0 = south edge, 1 = north
 * edge.  A halo is lb_halo_floats() = 18*nx floats: 18 row segments, three rows deep (what the
 * three-step kernel needs; a superset of what the two- and single-step kernels read):
 *   north edge out / south ghost in: row H-3 (resp. -3): k=2,5,6; row H-2 (resp. -2): k=0,1,3,2,5,6;
 *                                    row H-1 (resp. -1): k=0..8
 *   south edge out / north ghost in: row 0 (resp. H): k=0..8; row 1 (resp. H+1): k=0,1,3,4,7,8;
 *                                    row 2 (resp. H+2): k=4,7,8
 * export copies the edge rows into buf, import copies buf into the ghost rows; the buffer a slab
 * exports on its north side is what its northern neighbour imports on its south side.  buf may be
 * host or device memory (hipMemcpyDefault). */
int lb_halo_floats(lb_sim *s);
int lb_halo_export(lb_sim *s, int side, void *buf);
int lb_halo_import(lb_sim *s, int side, const void *buf);
/* Obstacle-mask rows of the neighbouring slabs next to this one: south_rows = global rows
 * y0-LB_MASK_HALO_ROWS .. y0-1 (nearest last), north_rows = rows y0+H .. y0+H+LB_MASK_HALO_ROWS-1 (nearest
 * first), each [LB_MASK_HALO_ROWS][nx] int32, NULL = no solid cells.  The multi-step kernels recompute
 * the neighbours' edge rows and need their masks. */
int lb_set_mask_halo(lb_sim *s, const int32_t *south_rows, const int32_t *north_rows);
/* Advance `count` slab handles that tile one grid on ONE device in lock step: the multi-GPU schedule and kernels
 * without a second GPU (verification).  Halos move through the pack / unpack kernels of the RCCL path, the receiver
 * reading the sender's buffer; the members' streams are ordered by events alone, as lb_run's are (lb_set_debug_sync adds device joins for diagnosis). */
int lb_run_group(lb_sim **sims, int count, int n_steps);

/* Population sets (the periodic multi-population lattices of the reference's research forks: porous_media/
 * single_component.cl:338-375 `move_periodic` streams population `cur_field` of a [jumper][population][y][x] array with
 * periodic wrap; single_component.py:679-751 steps every population per iteration).  `count` (<= 8) whole-grid PERIODIC
 * handles of one geometry on one device, one per population, each with its own omega, advance n_steps in lock step
 * with ONE fused launch per time step for all of them.  Bitwise equal to lb_run on each handle. */
int lb_run_batch(lb_sim **sims, int count, int n_steps);

/* Coupled scalar lattices (the competing concentrations of the reference's advecting_range_expansion fork:
 * deterministic_fisher_waves.py runs five launches and five host waits per step, each looping over the fields in every
 * work-item).  `count` = 1 ... 4 LB_SEM_MULTIFIELD handles of one geometry, boundary family, layout flag and device, one per
 * field, each with its own omega and G (lb_set_reaction), advance n_steps in lock step with ONE fused launch per time step:
 * per cell rho_i = sum f of every field, rho_tot = rho_0 + rho_1 + ... in the order of `fields`, then field i relaxes towards
 * its linear equilibrium and grows by w_k G_i rho_i (1 - rho_tot).  The imposed velocity read is that of fields[0] for
 * every field (the fork has one u, v for all; Coupled_Scalars writes the same to every member).  The last launch stores every
 * field's rho.  lb_run on such a handle is the set of one.
 * lb_collide_coupled: the fork's un-fused collide_particles over the set -- every member's stored feq and rho, rho_tot summed
 * over the members' stored rho in order; lb_collide_particles on one such handle is the set of one.  The other phase entry
 * points work per handle (lb_move_bcs: the in-place bounce-back of LB_BC_BOX). */
int lb_run_coupled(lb_sim **fields, int count, int n_steps);
int lb_collide_coupled(lb_sim **fields, int count);

/* RCCL point-to-point halo exchange over xGMI, one rank per GPU.  Rank r owns
 * slab r; neighbours are r-1 (south) and r+1 (north), wrapping for PERIODIC.
 * unique_id is the 128-byte ncclUniqueId: rank 0 obtains it with
 * lb_comm_unique_id and the caller broadcasts it (torch.distributed).
 * lb_comm_init is collective (every rank of the communicator calls it: the ranks agree on the smallest
 * slab height there, which decides the kernels and the exchange rhythm).  lb_check(across_ranks = 1) is the only
 * other collective (two all-reduces of three scalars, outside the data path).  Afterwards lb_run on a slab
 * handle exchanges halos itself: two seven- / six-step (large slabs of >= 112 / 96 rows), five-step (>= 80 rows), four-step
 * (>= 64 rows) or three-step (>= 32 rows) launches per exchange with ghost zones 14 / 12 / 10 / 8 / 6 rows deep when nx >= 512,
 * otherwise one exchange of the 3-deep halo per launch. */
int lb_comm_available(void);               /* 0 when librccl can be loaded in this process (no communicator is made) */
int lb_comm_unique_id(void *unique_id_128);
int lb_comm_init(lb_sim *s, const void *unique_id_128, int rank, int nranks);

/* Peer transport: the halo rows are stored DIRECTLY into the neighbours' ghost rows, through device memory mapped from
 * one rank's process into the other's (hipIpcMemHandle; over xGMI between GPUs, plain device memory between processes that
 * share a GPU), and the ranks meet at device-side flags (sequence numbers in fine-grained device memory, written with
 * system-scope release stores by the neighbour's kernels, polled by one lane) -- no packing, no unpacking, no library
 * call on the data path, nothing the host waits for: the alternative SURVEY.md section 8(e) lists beside RCCL (the
 * reference itself is single-device: opencl_dim.py:229-240).  lb_run's schedule is the one it runs over RCCL.
 *   lb_peer_export   fills LB_PEER_HANDLE_BYTES with this handle's descriptor (IPC handles of its two lattices and its
 *                    flag block, its geometry).  The caller carries it to the two neighbouring ranks by any means
 *                    (torch.distributed all_gather of bytes, a file, a pipe).
 *   lb_peer_connect  maps the neighbours (NULL = wall; south = rank-1, north = rank+1, wrapping for PERIODIC; a
 *                    descriptor exported by THIS process is used in place, so a 1-rank periodic ring talks to itself) and
 *                    switches lb_run on this handle to the peer transport.  min_h = the smallest slab height over all ranks
 *                    (decides the kernels and the exchange rhythm; every rank passes the same number).  Not a collective by
 *                    itself, but every rank must have exported before anyone connects, and all ranks must call lb_run with
 *                    the same step counts (as over RCCL).
 * A rank whose neighbour does not arrive within LB_PEER_TIMEOUT_S seconds (environment, default 20) gives up waiting on
 * the device, and the next lb_sync / lb_check on that handle fails with LB_ERR_COMM.  One handle per process and GPU (a
 * handle waits on the device for its neighbours' kernels: several such handles in ONE process could share a hardware
 * queue and wait for each other forever -- lb_run_group is the in-process stand-in). */
#define LB_PEER_HANDLE_BYTES 384
int lb_peer_export(lb_sim *s, void *handle_out);
int lb_peer_connect(lb_sim *s, int rank, int nranks, const void *south_handle, const void *north_handle, int min_h);

/* ---- health check (the reference's forks warn when max |u| exceeds a tenth of the speed of sound,
 *      porous_media/single_component.py:221-225, and print field sums while debugging, check_fields() :753-766; the
 *      `dimensionless` classes have nothing, and a diverged run is only noticed after downloading a field) ------------
 * One device pass over the current populations of this handle's rows: the number of cells whose density or velocity is
 * not finite, the largest Mach number max |u| / c_s (c_s = 1/sqrt(3); velocity = first moment / density in every
 * semantics) and the total mass, sum of rho, over the finite cells.  Reduced on the device (wave64 cross-lane
 * reduction, one partial per workgroup, folded in a fixed order: the result is reproducible), 24 bytes travel to the
 * host.  Waits for the handle's work.  across_ranks != 0 on a handle with a communicator (lb_comm_init): the three
 * values are combined over all ranks with ncclAllReduce (sum, max, sum) -- a collective, every rank calls it.
 * Any output pointer may be NULL. */
int lb_check(lb_sim *s, int across_ranks, int64_t *n_nonfinite, float *max_mach, double *sum_rho);
/* lb_run_group joins the device at chosen points (bits: 1 after every launch phase, 2 after every exchange, 4 after every
 * step, 8 at entry and exit); 0 = events only, the schedule lb_run itself relies on.  Process-wide; initial value from the
 * environment variable LB_DEBUG_SYNC, default 0.  Returns the previous value. */
int lb_set_debug_sync(int bits);

/* ---- measurement --------------------------------------------------------- */
/* hipEvent pair on the handle's stream: start, [enqueue work], stop -> ms. */
int lb_timer_start(lb_sim *s);
int lb_timer_stop(lb_sim *s, float *elapsed_ms);
/* Device layout facts for DESIGN.md / bench.py: pitch = padded row width (floats) = row pitch of rho, u, v and (bytes) of
 * the mask; plane stride (floats) of the lattices: = pitch with interleaved rows (element (k, y, x) at
 * (y * 9 + k) * pitch + x), = (local_ny + 28) * pitch with LB_FLAG_PLANAR; bytes allocated. */
int lb_layout(lb_sim *s, int64_t *pitch, int64_t *plane_stride, int64_t *bytes_allocated);
/* Time steps advanced by one launch of the hot kernel in lb_run with the current variant / tuning:
 * 7 ... 2 when a seven- ... two-steps-per-pass kernel is in use, else 1 (bench.py prices a launch
 * with it). */
int lb_steps_per_launch(lb_sim *s);
/* How lb_run(n_steps) on a whole-grid OpenCL-path GPU handle splits the run into launches with the current variant / tuning:
 * returns the number of launches and writes the time steps of each (in launch order) into depths[0 .. max_launches-1] (NULL:
 * count only).  Every launch of a marching kernel moves the same bytes, so bench.py prices a block of K steps by its launches.
 * LB_ERR_STATE (no message) on slab, Cython-path and CPU handles. */
int lb_plan_launches(lb_sim *s, int n_steps, int *depths, int max_launches);
/* Name of that kernel, e.g. "k_deep<7> (...)<PERIODIC>", written into buf (NUL-terminated, truncated to buflen). */
int lb_hot_kernel(lb_sim *s, char *buf, int buflen);
/* Pick the fastest configuration of the fused kernels for THIS grid by timing each candidate on a few
 * live time steps (all candidates give bitwise identical results, so this simply advances the
 * simulation): returns the number of steps advanced (0 when there is nothing to choose -- also under a variant forced with
 * lb_set_variant, which fixes the kernels), <0 on error.
 * Blocks the host (it reads HIP event times).  lb_run never tunes by itself.  A runner-up within 5 % of the winner is timed against it
 * once more over longer samples.  With LB_TUNE_CACHE set (below) a result remembered for this shape is taken over instead (returns 0). */
int lb_autotune(lb_sim *s);
/* The same with one sample per candidate, for callers that are about to run max_steps steps anyway and
 * will wait for them (the Python classes' blocking run()): tunes only when the handle is untuned, the
 * variant automatic and the pass (361 steps; 889 on grids <= 768^2) fits into max_steps; returns the number
 * of steps advanced, 0 when it did nothing, and never more than max_steps: the longer comparison of a runner-up
 * within 5 % (lb_autotune's) is made only when max_steps has room for it as well.
 *
 * Environment: LB_TUNE_CACHE=<file> (or "mem": this process only) remembers every result of lb_autotune / lb_autotune_quick under
 * the handle's shape (GPU, grid, rows owned, boundary family, mask or not, layout flags, semantics; one text line each) and lets the
 * first lb_run / lb_autotune_quick of a later handle of that shape take it over -- kernel, waves per CU and the measured launch
 * costs lb_plan_launches splits runs by -- without spending a step on tuning.  Unset (the default): every handle starts from the
 * size heuristic.  Only speed depends on it: every candidate gives the same bits. */
int lb_autotune_quick(lb_sim *s, int max_steps);
/* Calibration launch: a plain 16-byte-per-lane copy of the current lattice into the other one
 * (which is scratch between steps).  *bytes_moved = bytes read + written.  Known traffic in the
 * fused kernel's access shape: corrects rocprofv3 FETCH_SIZE on gfx950 and gives the device's
 * own streaming ceiling. */
int lb_copy_calibration(lb_sim *s, int nontemporal, int64_t *bytes_moved);
/* Bits of the kernel variant word of lb_set_variant (below).  A marching kernel of k steps per pass is taken only with every
 * shallower one: the word for k_step5 is LB_VAR_STEP2 | LB_VAR_STEP3 | LB_VAR_STEP4 | LB_VAR_STEP5.  The values are part of the ABI
 * (LB_D2Q9/variants.py carries the same names for Python). */
typedef enum {
    LB_VAR_NT_STORES = 1 << 0,          /* non-temporal stores */
    LB_VAR_NT_LOADS = 1 << 1,           /* non-temporal loads (k_step) */
    LB_VAR_ROWS = 3 << 2,               /* field: rows per workgroup of k_step: 0 -> 4, LB_VAR_ROWS_1 -> 1, LB_VAR_ROWS_2 -> 2 */
    LB_VAR_ROWS_1 = 1 << 2,
    LB_VAR_ROWS_2 = 2 << 2,
    LB_VAR_XCD_ORDER = 1 << 4,          /* XCD-aware tile order (k_step) */
    LB_VAR_STEP2 = 1 << 5,              /* two time steps per pass where applicable (nx >= 512) */
    LB_VAR_STEP3 = 1 << 6,              /* three time steps per pass */
    LB_VAR_NO_CYCLE = 1 << 7,           /* slabs exchange their halo after every launch instead of every two (no halo cycle) */
    LB_VAR_STEP4 = 1 << 8,              /* four time steps per pass (nx >= 512; whole-grid handles of >= 128 rows, slabs of >= 64) */
    LB_VAR_TILES = 1 << 9,              /* four time steps per pass through 32 x 16 LDS tiles (k_tile4: whole-grid handles of
                                         * >= 64 x 64 cells; for small grids) */
    LB_VAR_STEP4_NO_AHEAD = 1 << 10,    /* A/B switch of a thing on by default: k_step4 without its one-row-ahead gather; a noisy
                                         * scalar lattice with LB_VAR_TILES: k_ad_tile4 draws per cell, without its noise plane in LDS */
    LB_VAR_NO_PRIO_TURNS = 1 << 11,     /* A/B switch of a thing on by default: k_step4 / k_step5 without the priority turns of
                                         * the two waves of a SIMD */
    LB_VAR_STEP5 = 1 << 12,             /* five time steps per pass on overlapping strips (k_step5: whole-grid handles where
                                         * LB_VAR_STEP4 applies and slabs of >= 80 rows -- the ten-step halo cycle; what the
                                         * automatic choice takes from 1200^2 periodic / 1850^2 walled cells of a whole grid,
                                         * 1280^2 cells of a slab or of the velocity-inlet family) */
    LB_VAR_TILE_LAUNCH_ORDER = 1 << 13, /* A/B switch of a thing on by default: k_tile4 takes its tiles in launch order instead
                                         * of one band of tile rows per XCD */
    LB_VAR_STEP6 = 1 << 14,             /* six time steps per pass (k_deep<6>, one wave per SIMD: whole-grid handles and slabs of
                                         * >= 96 rows -- the twelve-step halo cycle --, not the velocity-inlet family; automatic
                                         * from 1100^2 periodic (1250^2 with obstacle-mask cells; slabs: 2400^2) / 1700^2 walled
                                         * (slabs: 3800^2) cells) */
    LB_VAR_STEP7 = 1 << 15,             /* with LB_VAR_STEP6: seven time steps per pass (k_deep<7>: as k_deep<6>, slabs of >= 112
                                         * rows -- the fourteen-step halo cycle; automatic where six are, in a periodic whole grid
                                         * without a mask from 1900^2 cells) */
    LB_VAR_DEEP2 = 1 << 16              /* with LB_VAR_STEP6 | LB_VAR_STEP7: the seven-step launches by k_deep2 -- two waves per
                                         * strip and direction, two waves per SIMD (round 6; automatic on walled whole grids of
                                         * 1700^2 ... 2900^2 cells, one of lb_autotune's candidates) */
} lb_variant_bits;
/* Kernel variant selector for tuning experiments: -1 = automatic (default); otherwise an OR of lb_variant_bits.  Results never
 * depend on it (bitwise); the ranks of one run must use the same value. */
int lb_set_variant(lb_sim *s, int variant);
/* Slab handles (round 6; new work, the reference is single-device: opencl_dim.py:229-240).  Depth of the fused kernel the halo cycle
 * of lb_run runs on (the cycle is 2 x depth time steps between two exchanges): 0 = automatic (the size thresholds of
 * LB_VAR_STEP5, LB_VAR_STEP6, LB_VAR_STEP7), 3 ... 7 = that depth wherever the smallest slab of the run has >= 16 x depth rows, 8 = seven
 * steps per launch by k_deep2<7> (two waves per strip and direction, in pairs per SIMD) instead of k_deep<7> (lone waves: RCCL's
 * send / receive kernel slows the launches it runs beside by 5-30 %; k_deep2's do not run longer for it).  With 0 the
 * seven-step cycle runs on k_deep2 under the RCCL transport and on k_deep otherwise.  Results never depend on it (bitwise); EVERY
 * rank of a run must set the same value -- the ranks time the candidates together and agree (LB_D2Q9/slabs.py:
 * DistributedSlab.autotune). */
int lb_set_slab_cycle(lb_sim *s, int depth);
/* Where the halo exchange of a cycle runs (slabs; ABI 10).  0, the default: on the handle's communication stream, beside the second
 * interior launch and the inner part of the edge bands -- hidden, if its kernels find room beside kernels that fill the chip.  1: on the
 * COMPUTE stream, behind the second interior launch and in front of the next first one -- exposed (pack + transfer + unpack, ~45 us of a
 * self-exchange) but beside nothing.  RCCL's send / receive kernel (59 workgroups with 20 KB of LDS each) takes 15 us alone and up to a
 * whole launch beside k_deep, which it slows by 5-30 %; which placement wins depends on the slab's height and on the link, so the ranks
 * time both together and agree (DistributedSlab.autotune).  Results never depend on it (bitwise); every rank sets the same value.
 * Whole-grid handles and the CPU backend ignore it. */
int lb_set_exchange_inline(lb_sim *s, int on);
/* Diagnosis of a multi-GPU run.  lb_exchange_timing(s, 1) brackets every halo exchange of lb_run with a pair of timing events on the
 * stream that carries it (up to 256 exchanges between two queries; more are counted as dropped, not timed); lb_exchange_stats waits
 * for the exchanges recorded so far and returns their number, their total and longest duration in milliseconds -- pack / push, the
 * transfer, the wait for the neighbours' matching calls, unpack --, the depth of the halo cycle in use and the rows of one edge band
 * of its second launch (2 x depth + the extra rows that keep the band's waves busy as long as the interior's, plan.cpp:
 * band_extra), then starts over.  The bands are split -- only their outer 2 x depth rows wait for the exchange, which runs on a stream
 * of its own beside the rest --, so an exchange delays the compute stream once it takes longer than about a whole launch; bench.py
 * --gpus N prints the figures per rank.  (The three streams of a slab handle must not share a hardware queue: a process that creates
 * many streams wants GPU_MAX_HW_QUEUES=8 set before the HIP runtime loads -- INTEGRATION.md.) */
int lb_exchange_timing(lb_sim *s, int enable);
int lb_exchange_stats(lb_sim *s, int64_t *n_exchanges, double *total_ms, double *max_ms, int *cycle_depth, int *band_rows);

/* ---- the spectral screened-Poisson solver (the reference's spectral_poisson/screened_poisson.py: gpyfft plans and whole-array
 *      passes with a host wait behind each; reaction_diffusion/screened_poisson_waves.py couples it to a scalar lattice) ------------
 * An lb_spectral is NOT a handle kind (no semantics value, no lb_create): a periodic nx x ny box of complex float32, three arrays --
 * charge, xgrad, ygrad -- laid out [ny][nx], interleaved (re, im), and a screening length lambda.  It solves
 * (1 - lambda^2 laplace) phi = charge and returns grad phi, with the reference's conventions: wave indices are the integers of
 * numpy's fftfreq (the Nyquist index of an even axis is -n/2), the gradient multipliers are 2 pi i kx and 2 pi i ky, the inverse
 * carries 1 / (nx ny).  Each axis has 1 ... 4096 points and no prime factor other than 2, 3 and 5; any other length is refused with
 * LB_ERR_ARG before a device is touched.  The transform is the library's own (LDS Stockham passes of radix 5, 3, 4, 2; csrc/
 * kernels_spectral.h); work is enqueued on the solver's own stream, lb_spectral_get waits for it. */
typedef struct lb_spectral lb_spectral;
typedef enum { LB_SPECTRAL_CHARGE = 0, LB_SPECTRAL_XGRAD = 1, LB_SPECTRAL_YGRAD = 2 } lb_spectral_array;
int lb_spectral_create(int nx, int ny, int device, double lam, lb_spectral **out);
int lb_spectral_destroy(lb_spectral *sp);
int lb_spectral_set_lambda(lb_spectral *sp, double lam);
/* re_im: 2 nx ny floats on the host, or (on_device != 0) on the solver's device */
int lb_spectral_set(lb_spectral *sp, int which, const float *re_im, int on_device);
int lb_spectral_get(lb_spectral *sp, int which, float *re_im);
/* The phases of the reference, one by one.  lb_spectral_transform: the 2-D transform of one array in place (forward: rows, then
 * columns; inverse: columns, then rows and 1 / (nx ny)).  lb_spectral_screen: charge /= lambda^2 (kx^2 + ky^2) + 1.
 * lb_spectral_grad_multiply: xgrad = 2 pi i kx charge, ygrad = 2 pi i ky charge. */
int lb_spectral_transform(lb_spectral *sp, int which, int forward);
int lb_spectral_screen(lb_spectral *sp);
int lb_spectral_grad_multiply(lb_spectral *sp);
/* The whole solve in three launches (x-FFT of the rows; per block of columns the y-FFT, the screening, both multipliers and two
 * inverse y-FFTs in LDS; the inverse x-FFT of both gradients): charge ends as the screened spectrum, xgrad and ygrad as the complex
 * gradients, BITWISE what transform(charge, 1), screen, grad_multiply, transform(xgrad, 0), transform(ygrad, 0) leave. */
int lb_spectral_solve(lb_spectral *sp);
/* The solve with a scalar lattice's density as the charge and its velocity as the result: s is a whole-grid LB_SEM_DIFFUSION GPU
 * handle (either family) of the solver's grid and device.  streamed = 0: the charge is the handle's stored rho; 1: the density the
 * populations will have after streaming, which one launch (k_ad_moments) stores in the handle's rho first, moving nothing.  u and v
 * of s become scale x Re xgrad, scale x Re ygrad -- bitwise the float32 product with lb_spectral_solve's gradients --, cells x < nx
 * only; the solver's xgrad and ygrad are left half transformed.  On s's stream, behind the solver's own work, without a host wait;
 * feq of s is no longer current. */
int lb_spectral_velocity(lb_spectral *sp, lb_sim *s, float scale, int streamed);
/* n_steps times: k_ad_moments, the three launches of the solve, k_ad_step (never the LDS tiles: the velocity changes every step);
 * only the last step stores rho.  No host wait.  BITWISE n_steps x (lb_spectral_velocity(sp, s, scale, 1); lb_run(s, 1)). */
int lb_run_screened(lb_spectral *sp, lb_sim *s, float scale, int n_steps);

/* ---- a population and the nutrient it eats under the solver's velocity (the reference's reaction_diffusion/
 *      surfactant_nutrient_waves.py and .cl: Surfactant_Nutrient_Wave and Clumpy_Surfactant_Nutrient_Wave) ----------------------------
 * NOT a handle kind either: a set is exactly two whole-grid LB_SEM_DIFFUSION, LB_BC_PERIODIC GPU handles of one geometry, layout flag
 * and device -- fields[0] the population p, fields[1] the nutrient n, each with its own omega -- and an lb_spectral of their grid.
 * The parameters travel with every call; nothing is stored in a handle except psi and F, which live with the first member, are made
 * at first use and freed by lb_destroy.  LB_ERR_ARG, with the reason, before any launch: a count other than 2, a handle given twice,
 * a member that is no scalar lattice on the GPU or not periodic, members of different geometry, layout or device, a grid the solver
 * was not created for, non-finite parameters, clumpy with nx or ny < 3 or with rho_o == 0, a negative n_steps; LB_ERR_STATE for slabs.  With cs = float32(1 / sqrt(3)) and 1 / cs^2 = float32(1. / (cs cs)) in the force term (the convention of the
 * colonies above), one time step (surfactant_nutrient_waves.py: run) is
 *   1. both lattices stream, periodic wrap (move_periodic + copy)                                              lb_move on each member
 *   2. rho_i = sum_k f_ik                                                                                      lb_update_hydro on each
 *   3. (u, v) = scale Re grad phi, (1 - lam^2 laplace) phi = rho_p; one velocity for both (update_u_and_v)     lb_nutrient_velocity
 *   4. clumpy: psi = rho_o (1 - exp(-max(rho_p, 0) / rho_o)),                                                  lb_update_forces_nutrient
 *        F = ((-cs cs) G_chen) psi(x) sum_k w_k c_k psi(x + c_k), periodic wrap
 *   5. feq_ik = w_k rho_i (1 + c_k.u / cs^2)                                                                   lb_update_feq on each
 *   6. population: f_k (1 - omega) + omega feq_k + w_k G rho_p rho_n [clumpy: + (w_k c_k.F) / cs^2];           lb_collide_nutrient
 *      nutrient:   f_k (1 - omega_n) + omega_n feq_k - w_k G rho_p rho_n.  No floor at zero.
 * lb_run_nutrient(n) = n steps on the first member's stream without a host wait, of FIVE launches each: k_ad_moments on the
 * population (its density after streaming, nothing moved), the three launches of the solve, and k_sn_step, which gathers both
 * lattices, relaxes them with the scalar lattice's cell arithmetic (with G = 0, scale = 0 and clumpy = 0 a member gets k_ad_step's
 * bits) and, clumpy, stages psi of a workgroup's rows and their halo in LDS.  It leaves f post-collision, rho, u, v (on both
 * members), psi and F those of the last step before its collision, feq not current.  The fused step and the stages are held to each
 * other by the contract's tolerance, not bitwise: the stages store feq, the fused cell lets omega enter through rho (as lb_run and the
 * phases of a scalar lattice differ). */
typedef struct { float G, scale; int32_t clumpy; float rho_o, G_chen; } lb_nutrient_params;   /* clumpy: rho_o != 0 */
int lb_run_nutrient(lb_spectral *sp, lb_sim **fields, int count, const lb_nutrient_params *p, int n_steps);
/* stage 3: lb_spectral_velocity on fields[0] (streamed as there), then u, v copied into fields[1] device to device, same stream */
int lb_nutrient_velocity(lb_spectral *sp, lb_sim **fields, int count, float scale, int streamed);
int lb_update_forces_nutrient(lb_sim **fields, int count, const lb_nutrient_params *p);      /* stage 4 from the stored rho_p (clumpy only) */
int lb_collide_nutrient(lb_sim **fields, int count, const lb_nutrient_params *p);            /* stage 6: stored feq, rho, F */
/* psi, Fx, Fy of the last step / the last lb_update_forces_nutrient: [ny][nx] each, any may be NULL; zero before either */
int lb_get_nutrient_fields(lb_sim **fields, int count, float *psi, float *Fx, float *Fy);

/* ---- noisy strains on a shared nutrient (the reference's advecting_range_expansion/stochastic_nutrients.py: Expansion, and
 *      D2Q9_multifield_diffusion.cl) ---------------------------------------------------------------------------------------------------
 * NOT a handle kind either: a set is count = 2 ... 4 whole-grid LB_SEM_DIFFUSION GPU handles of one geometry, layout flag, device and
 * family -- LB_BC_OPEN, the reference's box with each member's own edge state, or LB_BC_PERIODIC.  fields[0 .. count-2] are the
 * strains, fields[count-1] is the nutrient.  Per strain: omega from its parameters, G from lb_set_reaction, Dg, seed and the noise
 * counter t from lb_set_noise.  The nutrient has its own omega, G == 0 and no noise.  zero_cutoff travels with every call; nothing is
 * stored in a handle and nothing new is allocated.  The velocity every member reads is the first member's u, v.  One time step
 * (stochastic_nutrients.py:478-496), with c the nutrient's rho:
 *   1. every member streams; OPEN: a link that would enter from outside keeps the edge state (move + copy_buffer)   lb_move on each
 *   2. rho_i = sum_k f_ik, left to right; rho_i < zero_cutoff or NaN: rho_i = 0 (update_hydro)                     lb_update_hydro_expansion
 *   3. feq_ik = w_k rho_i (1 + 3 c_k.u) of the stored rho (update_feq)                                             lb_update_feq on each
 *   4. strain i: react_i = (G_i rho_i) c + sqrt((Dg_i rho_i) c) z_i + ((Dg_i c) / 4)(z_i z_i - 1),                 lb_collide_expansion
 *        f_ik = f_ik (1 - omega_i) + omega_i feq_ik + w_k react_i;
 *      nutrient: ... - w_k sum_i react_i, accumulated in the strains' order;
 *      a link becomes 0 where its member's rho < zero_cutoff, where the new value is < 0 or where it is NaN (collide_particles)
 *   5. z_i is strain i's own stream at its noise counter t, as lb_noise_fill gives it; every noisy strain's t advances by one.  A
 *      strain with Dg == 0 draws nothing and its t does not move.
 * lb_run_expansion(n) = n steps on the first member's stream without a host wait, ONE launch each (k_ex_step: every member gathered,
 * the normals drawn in registers); each member's variant is ignored.  It leaves f post-collision and rho, u, v of the last step, feq
 * not current.  The fused step and the stages are held to each other by the contract's tolerance, not bitwise (as lb_run and the phases
 * of a scalar lattice differ).  lb_collide_expansion takes z_i from the strain's supplied field where lb_set_noise_field set one.
 * LB_ERR_ARG, with the reason, before any launch: a null array, handle or parameters, a count outside 2 ... 4, a handle given twice, a
 * member that is no scalar lattice on the GPU, a family other than OPEN or PERIODIC, members of different geometry, layout, device or
 * family, a non-finite zero_cutoff, a nutrient with G != 0, two noisy strains with equal seeds, a negative n_steps.  LB_ERR_STATE:
 * slabs, a noisy nutrient, lb_run_expansion while any member holds a supplied noise field, lb_collide_expansion before
 * lb_update_feq on every member. */
typedef struct { float zero_cutoff; } lb_expansion_params;
int lb_run_expansion(lb_sim **fields, int count, const lb_expansion_params *p, int n_steps);
int lb_update_hydro_expansion(lb_sim **fields, int count, const lb_expansion_params *p);     /* stage 2 */
int lb_collide_expansion(lb_sim **fields, int count, const lb_expansion_params *p);          /* stage 4: stored feq, rho */

/* ---- a flow and the scalars it carries (a dye, a temperature, a growing population under a live velocity field) ----------------------
 * NOT a handle kind either: `flow` is a whole-grid LB_SEM_OPENCL GPU handle of the family LB_BC_PERIODIC without an obstacle mask and
 * without LB_FLAG_HALO, scalars[0 .. count-1], count = 1 ... 2, are whole-grid LB_SEM_DIFFUSION GPU handles of the family LB_BC_PERIODIC
 * with the flow's nx, ny and device, the noisy collision off and no noise field set.  Every scalar keeps its own omega and its own G
 * (lb_set_reaction); LB_FLAG_PLANAR may be set on any member.  One time step: the flow streams and forms rho, u, v of every cell from its
 * streamed populations; every scalar streams and relaxes towards w_k rho_i (1 + 3 c_k.u) with THAT u, v -- the moments of the flow's
 * step t, what a LB_FLAG_EAGER_MACRO flow handle stores, not the velocity rebuilt from the post-collision populations, which differs by
 * rounding --; the flow relaxes.  lb_run_advected(n) is bitwise equal to n x (lb_run(flow, 1) on an eager flow handle; for each i
 * lb_set_velocity_from(scalars[i], flow) and lb_run(scalars[i], 1) under lb_set_variant(scalars[i], 0)).  Everything is enqueued on the
 * flow's stream, without a host wait; the scalars' streams are joined before and released behind.
 *   form 1: ONE launch per step (k_fa_step: every lattice gathered, u, v handed from the flow's collision to the scalars' in registers;
 *           72 (1 + count) B per cell and step);
 *   form 0: 1 + count launches per step (the flow's k_step with its rho, u, v epilogue, then one k_ad_step per scalar reading the flow
 *           handle's u, v planes: no copy; 84 + 80 count B);
 *   form -1: the planner's choice by grid size (advected_form, csrc/plan.cpp, from profiles/advected_bench.txt).  The same bits.
 * Afterwards the flow's rho, u, v are stored and current -- as on an eager handle, also on one that rebuilds them on demand --, every
 * scalar's rho is stored, every scalar's u, v hold the velocity of the last step, and feq is not current on any member.  n_steps == 0
 * does nothing.  lb_hot_kernel on the flow handle keeps naming lb_run's kernel; lb_advected_kernel names what lb_run_advected runs for
 * `count` scalars on a grid of `cells` cells under `form`.
 * LB_ERR_ARG, with the reason, before anything is enqueued: a null flow, array or member ("null"), a count outside 1 ... 2, a flow of
 * another kind, backend or family, a member that is no LB_SEM_DIFFUSION GPU handle (the flow itself or a field of a coupled set
 * included) or not periodic, a handle given twice, another grid or device, a form outside -1 ... 1, a negative n_steps.  LB_ERR_STATE:
 * slabs and LB_FLAG_HALO, a flow with an obstacle mask, a member inside a split step, a noisy scalar, a scalar with a noise field. */
int lb_run_advected(lb_sim *flow, lb_sim **scalars, int count, int n_steps, int form);
int lb_advected_kernel(int count, int form, int64_t cells, char *buf, int buflen);

#ifdef __cplusplus
}
#endif
#endif /* LB_HIP_H */
