/*
 * upkie_hip.h -- C-ABI of the MI355X-native batched Upkie simulation step.
 *
 * This is the drop-in boundary for the reference's backend plugin interface
 * (upkie/envs/backends/backend.py:11-50: reset / step / get_spine_observation
 * / close) batched over B independent environments. Every entry point takes
 * plain pointers and sizes; device pointers are owned by the caller (PyTorch
 * tensors on the Python side), launches go on the caller's hipStream_t and
 * nothing here synchronises the device. No exception crosses this boundary:
 * functions return 0 on success and a negative UpkieStatus on error, with a
 * message available from upkie_sim_last_error().
 *
 * Data layout (all device buffers, fp32):
 *   state    [UPKIE_STATE_WORDS][B]   struct-of-arrays, word index below
 *   act/obs  row-major [B][d] as gymnasium.vector would hand them over
 */
#ifndef UPKIE_HIP_H_
#define UPKIE_HIP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define UPKIE_NB 7 /* merged rigid bodies: trunk, L{thigh,calf,wheel}, R{..} */
#define UPKIE_NJ 6 /* actuated joints, reference order (static_config.h:64-69,
                      kinematic_tree.py:105-127): left_hip, left_knee,
                      left_wheel, right_hip, right_knee, right_wheel */

/* ---- per-env state words (SoA rows of the state buffer) ---------------- */
enum UpkieStateWord {
  UPKIE_S_POS = 0,      /* 3: base position in world                        */
  UPKIE_S_QUAT = 3,     /* 4: base->world quaternion (w, x, y, z)           */
  UPKIE_S_LINVEL = 7,   /* 3: base linear velocity, world frame             */
  UPKIE_S_ANGVEL = 10,  /* 3: base angular velocity, world frame            */
  UPKIE_S_Q = 13,       /* 6: joint angles                                  */
  UPKIE_S_QD = 19,      /* 6: joint velocities                              */
  UPKIE_S_LEGREF = 25,  /* 4: hip/knee low-pass targets (lh, lk, rh, rk),
                              upkie_gyropod.py:246-267                      */
  UPKIE_S_YAW = 29,     /* 1: integrated commanded yaw, upkie_gyropod.py:383 */
  UPKIE_S_YAWVEL = 30,  /* 1: last commanded yaw velocity                   */
  UPKIE_S_TORQUE = 31,  /* 6: last commanded joint torques (servo "torque"
                              observation, pybullet_backend.py:456-458)     */
  UPKIE_S_IMUVEL = 37,  /* 3: previous IMU linear velocity (world), for the
                              finite-difference accelerometer :405-408      */
  UPKIE_S_EPISODE = 40, /* 1: number of resets done so far (RNG stream id),
                              modulo 2^24 (UPKIE_COUNTER_MASK)              */
  UPKIE_S_DONE = 41,    /* 1: 1.0 when the env terminated and awaits reset  */
  UPKIE_S_MPC_V = 42,   /* 1: MPCBalancer.commanded_velocity                */
  UPKIE_S_SE2_X = 43,   /* 1: dead-reckoned x, upkie_base_velocity.py:197   */
  UPKIE_S_SE2_Y = 44,   /* 1: dead-reckoned y                               */
  UPKIE_S_CONTACT = 45, /* 1: floor contact flag after the last substep     */
  UPKIE_S_STEP = 46,    /* 1: env.step() calls so far (torque-noise stream),
                              modulo 2^24                                    */
  UPKIE_S_ELAPSED = 47, /* 1: steps of the current episode (time limit)      */
  UPKIE_STATE_WORDS = 48
};

/* The counters are held as fp32 VALUES (so that they read naturally from a
 * float tensor): exact up to 2^24, then they wrap to 0 instead of sticking. */
#define UPKIE_COUNTER_MASK 0xFFFFFFu

/* Words the fused Pendulum step reads and writes (29 physics/filter words +
 * the done flag); everything else is untouched by that kernel. */
#define UPKIE_PENDULUM_STATE_WORDS 29

/* URDF links the model remembers (upkie_description's Upkie has 15 with mass). */
#define UPKIE_MAX_LINKS 24
/* Per-env inertial record of one composite body: mass, com (3, body frame),
 * inertia about the com (xx yy zz xy xz yz, body axes). */
#define UPKIE_INERTIAL_WORDS 10

enum UpkieStatus {
  UPKIE_OK = 0,
  UPKIE_ERR_INVALID_ARGUMENT = -1,
  UPKIE_ERR_UNSUPPORTED_MODEL = -2,
  UPKIE_ERR_HIP = -3,
  UPKIE_ERR_NO_DEVICE = -4
};

enum UpkieAutoreset {
  UPKIE_AUTORESET_DISABLED = 0, /* caller resets through a mask             */
  UPKIE_AUTORESET_NEXT_STEP = 1 /* gymnasium.vector default: an env that
                                   terminated at step t is reset by step t+1,
                                   which ignores its action                 */
};

/* Merged-fixed-link rigid-body model. Body frames are located at their joint
 * origin and aligned with the base frame at the zero configuration, so the
 * tree transforms are pure translations (the host-side URDF loader does this
 * canonicalisation). Replaces what the reference gets from upkie_description's
 * URDF through pybullet.loadURDF (pybullet_backend.py:121-125) and
 * upkie/model/model.py:63-110. */
typedef struct UpkieModel {
  double mass[UPKIE_NB];
  double com[UPKIE_NB][3];        /* centre of mass in body frame           */
  double inertia[UPKIE_NB][6];    /* about the com: xx yy zz xy xz yz       */
  double joint_pos[UPKIE_NJ][3];  /* joint origin in the parent body frame  */
  double joint_axis[UPKIE_NJ][3]; /* unit rotation axis in body frame       */
  double joint_lower[UPKIE_NJ];
  double joint_upper[UPKIE_NJ];
  double joint_effort[UPKIE_NJ];   /* N.m   */
  double joint_velocity[UPKIE_NJ]; /* rad/s */
  double joint_damping[UPKIE_NJ];  /* URDF <dynamics damping>, N.m.s/rad    */
  double wheel_radius;             /* tire collision cylinder radius        */
  double wheel_center[2][3];       /* tire centre in the wheel body frame   */
  double wheel_base;               /* model.py:88 */
  double left_sign;                /* +1 if left-wheeled, model.py:104      */
  double imu_pos[3];               /* IMU origin in base frame              */
  double rot_base_to_imu[9];       /* row-major, model.py:106               */
  double gravity;                  /* 9.81, pybullet_backend.py:110         */
  double contact_stiffness;        /* tire <contact> stiffness              */
  double contact_damping;          /* tire <contact> damping                */
  double friction_mu;              /* tire x plane lateral friction         */
  double friction_cfm;             /* compliance added to friction rows, 1/kg:
                                      the two tires' lateral rows coincide in a
                                      symmetric stance (singular otherwise)  */
  double contact_breaking_threshold; /* floor_contact flag distance         */
  double base_linear_damping;      /* Bullet default 0.04                   */
  double base_angular_damping;     /* Bullet default 0.04                   */
  double max_joint_velocity;       /* Bullet maxCoordinateVelocity, 100     */
  double pgs_tolerance;            /* sweeps stop once no impulse moved by more
                                      than this fraction of the largest one;
                                      the fp32 kernels do not go below 1e-5  */
  int32_t pgs_iterations;          /* Bullet numSolverIterations, 50        */
  int32_t enforce_joint_limits;    /* hip/knee limit rows in the solver     */
  /* The URDF links each composite body was fused from: what Bullet keeps as
   * separate links (no URDF_MERGE_FIXED_LINKS, pybullet_backend.py:121-125) and
   * randomize_inertias() scales one by one (pybullet_backend.py:555-601).
   * num_links = 0: one link per body. */
  int32_t num_links;
  int32_t link_body[UPKIE_MAX_LINKS];       /* composite body of the link   */
  int32_t link_randomized[UPKIE_MAX_LINKS]; /* 0 for the URDF root link: Bullet's
                                               base (index -1) is not in
                                               range(getNumJoints), :563     */
  double link_mass[UPKIE_MAX_LINKS];
  double link_com[UPKIE_MAX_LINKS][3];      /* link com in its body's frame  */
  double link_inertia[UPKIE_MAX_LINKS][6];  /* about the link com, body axes:
                                               xx yy zz xy xz yz             */
} UpkieModel;

/* Everything gym.make(...) kwargs decide for one batch of environments
 * (entry_points.py:41-54,99-105; upkie_servos.py:115-124;
 * upkie_gyropod.py:104-111; joint_properties.py:4-40;
 * robot_state.py:52-120; robot_state_randomization.py:53-90). */
typedef struct UpkieSimConfig {
  int32_t num_envs;     /* B, envs hosted by this handle                    */
  int32_t nb_substeps;  /* int(1000 * dt) unless given, backend :85-87      */
  double dt;            /* 1 / frequency                                    */
  double torque_control_kp; /* 20.0 */
  double torque_control_kd; /* 1.0  */
  double joint_friction[UPKIE_NJ];           /* JointProperties.friction   */
  double torque_control_noise[UPKIE_NJ];     /* std dev, N.m               */
  double torque_measurement_noise[UPKIE_NJ]; /* std dev, N.m               */
  double fall_pitch;          /* 1.0 */
  double max_ground_velocity; /* 3.0 */
  double max_yaw_velocity;    /* 1.0 */
  double leg_gain_scale;      /* 1.0 */
  double max_gain_scale;      /* 5.0 */
  /* nominal initial state (RobotState) */
  double init_pos[3];
  double init_quat[4]; /* w x y z */
  double init_linvel[3];
  double init_angvel[3];
  double init_joint[UPKIE_NJ];
  /* RobotStateRandomization magnitudes */
  double rand_roll, rand_pitch, rand_x, rand_z, rand_omega_x, rand_omega_y;
  double rand_linvel[3];
  uint64_t seed;          /* Philox key                                     */
  int64_t env_id_offset;  /* global index of local env 0 (multi-GPU shards) */
  int32_t autoreset_mode; /* UpkieAutoreset                                 */
  int32_t max_episode_steps; /* gymnasium TimeLimit for the batch: the step that
                                brings an episode to this many steps reports
                                `truncated` (unless the robot fell in it) and
                                flags the env done; 0 = no limit            */
  /* Fused linear-feedback agent (README.md:62-64): a = clip(g . obs, +-c)  */
  double agent_gains[4];
  double agent_clip;
} UpkieSimConfig;

typedef struct UpkieSim UpkieSim;

/* Library / device probe. Returns the number of visible HIP devices (>= 0)
 * or a negative status. */
int upkie_hip_device_count(void);

/* sizeof() of a public struct AS THIS BUILD OF THE LIBRARY SEES IT (-1 for an
 * unknown id): a binding written against one version of this header checks it
 * against its own mirror of the struct before the first call -- the config
 * structs grow at the tail from release to release (UpkieMpcConfig gained
 * admm_relaxation), and a library loaded from elsewhere (UPKIE_HIP_LIBRARY)
 * that reads a longer struct than the caller wrote reads garbage silently.
 * upkie_amd/lib.py refuses to load a library whose sizes differ from
 * upkie_amd/abi.py's. No counterpart in the reference (its backends are
 * Python objects). */
enum UpkieStructId {
  UPKIE_STRUCT_MODEL = 0,
  UPKIE_STRUCT_SIM_CONFIG = 1,
  UPKIE_STRUCT_EXTERNAL_FORCES = 2,
  UPKIE_STRUCT_SERVO_POLICY = 3,
  UPKIE_STRUCT_SPINE_OBSERVATION = 4,
  UPKIE_STRUCT_MPC_CONFIG = 5,
  UPKIE_STRUCT_OBSERVER_CONFIG = 6,
  UPKIE_STRUCT_OBSERVER_INPUT = 7,
  UPKIE_STRUCT_OBSERVER_OUTPUT = 8,
  UPKIE_STRUCT_MLP_SHAPE = 9,
  UPKIE_STRUCT_PPO_CONFIG = 10,
  UPKIE_STRUCT_EPISODE_EVENTS = 11,
  UPKIE_STRUCT_TASK_TARGETS = 12,
  UPKIE_STRUCT_PPO_MIRROR = 13,
  UPKIE_STRUCT_COUNT = 14
};
int64_t upkie_hip_struct_bytes(int which);

/* Streams and hipGraphs. Every launching entry point takes the caller's
 * hipStream_t (`stream`, NULL = the default stream) and only enqueues work on
 * it. The eight-lane step kernels read the handle's limits and configuration
 * from a block in device memory, refreshed by a small store kernel enqueued in
 * front of the step whenever a setting changed (upkie_sim_set_config, ...) or
 * the launching stream did. What that allows:
 *   - eager launches: the handle keeps TWO such blocks and alternates, so the
 *     steps of one handle may be in flight on up to two streams at a time
 *     (a third stream must wait for the first to drain: the handle does not
 *     track completion);
 *   - launches recorded into a hipGraph (stream capture, e.g.
 *     torch.cuda.graph / upkie_amd.graphs): each CAPTURE gets a block of its
 *     own and records its own store of the settings as they are at capture
 *     time, so several graphs of one handle -- recorded at different settings,
 *     replayed in any order, mixed with eager launches -- each replay with the
 *     settings they were recorded with. The blocks are allocated with the
 *     handle (a capture cannot allocate): at most UPKIE_MAX_GRAPH_CAPTURES
 *     captures per handle, the next one is refused with UPKIE_ERR_HIP and a
 *     message. The library cannot see a graph being destroyed: a long-lived
 *     env that re-captures (after a setting change, after an aborted capture)
 *     hands the blocks back with upkie_sim_release_graph_captures() once none
 *     of the graphs recorded so far will be replayed again. A setting changed
 *     AFTER a capture does not reach that graph's replays: re-capture.
 * The one- and two-lane kernels take their settings by value: no limit. */
#define UPKIE_MAX_GRAPH_CAPTURES 8

/* Create a simulation handle on the current HIP device: validates the model
 * (all joint axes must be lateral, i.e. +-y of the base frame, as on every
 * Upkie; UPKIE_ERR_UNSUPPORTED_MODEL otherwise) and uploads constants.
 * Replaces PyBulletBackend.__init__ (pybullet_backend.py:55-197). */
int upkie_sim_create(const UpkieSimConfig* config, const UpkieModel* model,
                     UpkieSim** out);
int upkie_sim_destroy(UpkieSim* sim);
const char* upkie_sim_last_error(const UpkieSim* sim);
/* "Streams and hipGraphs" above: every hipGraph recorded from this handle so
 * far is dead to the caller; its settings blocks may be handed out again. */
int upkie_sim_release_graph_captures(UpkieSim* sim);

/* Replace the configuration of an existing handle (same num_envs): lets a
 * caller change init state, randomisation magnitudes, seed, gains, fall pitch
 * ... between resets, as the reference's mutable env attributes allow
 * (upkie_env.py:244-251 update_init_rand, upkie_gyropod.py:176-184). */
int upkie_sim_set_config(UpkieSim* sim, const UpkieSimConfig* config);

/* Size in bytes the caller must allocate for the state buffer. */
int64_t upkie_sim_state_bytes(const UpkieSim* sim);

/* The relative tolerance the Gauss-Seidel sweeps of this handle's kernels stop
 * at: UpkieModel.pgs_tolerance, but never below 1e-5 -- the kernels sweep in
 * fp32, where a six-term residual cannot be told from zero below that, and a
 * tighter setting only ran systems into the iteration cap (the fp64 oracle
 * honours the model's value). */
double upkie_sim_pgs_tolerance(const UpkieSim* sim);

/* Lanes of a wavefront that share one env in the step kernels of this handle:
 * chosen from the batch size at creation (small batches spread every env over
 * several lanes so that the chip's SIMDs all hold a wave; large ones keep one
 * env per lane), or forced by the environment variable UPKIE_LANES_PER_ENV
 * (tests, sweeps). Results agree across mappings to fp32 rounding -- where a
 * contact solution leaves its friction box, to the solver's tolerance: the
 * eight-lane kernel answers such substeps by an active-set solve, the others
 * by sweeps -- and bit for bit within one. */
int upkie_sim_lanes_per_env(const UpkieSim* sim);
/* ... of the step kernel a given entry point launches, named by the layout of
 * its observation output (UpkieObservationLayout): the Servos kernels, which
 * take the whole register file, leave the eight-lane mapping at 8192 envs, the
 * others at 16384 -- a caller that keys on the mapping (the census below is
 * counted by the eight-lane kernels only; the SAME_STEP autoreset runs inside
 * the launch there) asks for the entry point it uses. */
int upkie_sim_lanes_per_env_of(const UpkieSim* sim, int observation_layout);
/* Force the mapping of this handle's later launches: 1, 2 or 8 lanes per env,
 * 0 = back to the choice by batch size (what UPKIE_LANES_PER_ENV sets at
 * creation). A forced mapping still yields where it does not exist (the
 * eight-lane kernels beyond 2^32 bytes of state or with forces on leg links,
 * the two-lane kernels under the Bullet-like contact model). */
int upkie_sim_set_lanes_per_env(UpkieSim* sim, int lanes);

/* Non-finite commands and states. The reference has one robot and asserts
 * (`assert not np.isnan(target_velocity)`, pybullet_backend.py:519); a batch of
 * thousands must not stop -- nor keep a poisoned env for ever -- because one
 * policy output diverged. Every step entry point therefore
 *  1. replaces what is still NOT FINITE behind the reference's clamp
 *     (upkie_servos.py:331-342; only NaN survives a clamp, and an infinite
 *     position target of a joint without position limits) by the NEUTRAL
 *     action's value (upkie_servos.py:255-262): velocity 0, feedforward torque
 *     0, kp_scale 1, kd_scale 1, maximum_torque = the joint's effort limit; an
 *     infinite position becomes NaN, which is the neutral position ("no
 *     position term"). A NaN ground / yaw velocity action of the Pendulum /
 *     Gyropod / BaseVelocity steps is 0, an infinite yaw velocity -- the yaw
 *     word integrates the unclamped action, upkie_gyropod.py:383-385 -- is
 *     max_yaw_velocity with its sign; a non-finite target velocity of the MPC
 *     balancer is 0;
 *  2. looks at the env's state behind the substeps: if a word of it is not
 *     finite (a force, an inertial record or an uploaded state word was not),
 *     the env is put into UpkieSimConfig's initial state WITHOUT randomisation,
 *     at rest, its contact cache dropped; the step reports `terminated = 1`
 *     for it -- every env kind, UpkieServos included -- and flags it done, so
 *     the autoreset treats it like a fall (NEXT_STEP: re-initialised by its
 *     next step; SAME_STEP: inside this call; disabled: until the caller
 *     resets it). No NaN leaves a step in an observation.
 * Finite values, however large, go through the reference's arithmetic
 * untouched (its clamps bound them). Both events are counted per handle:
 * counts[0] = command words replaced, counts[1] = env states replaced since
 * creation (or the last call with reset != 0); the call waits for `stream`.
 * The sound envs pay about twenty compares per step for this. */
int upkie_sim_guard_counts(UpkieSim* sim, uint32_t counts[2], int reset, void* stream);

/* gymnasium's SAME_STEP autoreset completed by the step calls themselves: with
 * `final_obs` set (a device buffer shaped like the step's observation output:
 * [B][4] Pendulum, [B][6] Gyropod, [B][6][5] Servos) and
 * UpkieSimConfig::autoreset_mode == UPKIE_AUTORESET_DISABLED (no NEXT_STEP reset),
 * upkie_sim_step_pendulum / _gyropod / _servos return with every env's last
 * observation in `final_obs`, the finished envs re-initialised and their rows
 * of the observation output replaced by the reset observation (reward and flags
 * are those of the step) -- what upkie_sim_autoreset_done does as a second call,
 * inside the same launch where the lane mapping allows it (batches up to 8192
 * envs), as a second launch otherwise. NULL (the default): the step calls only
 * flag the finished envs. Mirrors gymnasium.vector's AutoresetMode.SAME_STEP
 * (the reference's envs are single robots: no counterpart there). */
int upkie_sim_set_final_observation(UpkieSim* sim, float* final_obs);

/* Contact model. Default (`manifold` NULL): the product's specification -- one
 * contact point per tire, exact solve; when the solution leaves the friction
 * box, an active-set solve (eight-lane kernel) and Gauss-Seidel sweeps to
 * convergence, friction CFM 0.01. With `manifold` set -- the caller's device buffer
 * [UPKIE_CONTACT_MANIFOLD_WORDS][B] fp32, zeroed by the caller, kept between
 * steps -- every step of this handle solves contacts and joint limits the way
 * Bullet's multibody solver is published to inside pybullet.stepSimulation()
 * (call sites pybullet_backend.py:228,306; third
 * party, absent here: restated, unverified): a persistent manifold of up to
 * four points per tire (refresh against the breaking threshold, nearest cached
 * point replaced), one normal + two friction rows per point along / across
 * its sliding velocity, no friction CFM, a FIXED number of sequential-impulse
 * sweeps (UpkieModel.pgs_iterations = 50; joint limits, normals, then each
 * point's friction pair projected onto the cone), normal impulses warm-started
 * with 0.85 x the last applied ones. Per env and tire four records of 8 words:
 * point in the wheel frame (3), on the plane in world coordinates (3), applied
 * normal impulse, live flag. A reset clears an env's manifold. Two kernels run
 * this model: the one-env-per-lane step kernels cover every case (several
 * points on a tire, joints at their stops in the same solve, any batch size,
 * every entry point); up to 16384 envs (upkie_sim_step_servos: 8192) the step
 * entry points run it on eight lanes per env, in the case a rolling wheel
 * produces (one cached point per tire, which the tire's deepest point replaces
 * every substep: the default model's contact point with the friction rows
 * rotated into the sliding direction; a robot lying flat on its side, whose
 * tires may cache several points under Bullet's rule, keeps the deepest one
 * on this variant -- upkie_sim_set_lanes_per_env(sim, 1) selects the one-lane
 * kernels; a joint within reach of its stop is a row of the same 50 sweeps on
 * both, since round 6 -- until then the eight-lane variant answered such a
 * substep with the default model's joint-stop solve --, and is counted by the
 * census, word [0]).
 * Both keep complete manifold records, so either continues from a manifold the
 * other wrote. About 2.3 x the default model's Pendulum step (the sweeps are ~36 packed-
 * fp32 instructions each); the default stays the product's fast
 * specification. This is the model to answer "what would PyBullet's contact
 * pipeline do", e.g. the first thing tools/compare_with_pybullet.py holds
 * against the real thing. */
#define UPKIE_CONTACT_MANIFOLD_WORDS 64
int upkie_sim_set_contact_manifold(UpkieSim* sim, float* manifold);

/* Rare-path census of the eight-lanes-per-env step kernel (octet.hpp): `counters`
 * is the caller's device buffer of UPKIE_CENSUS_WORDS uint32 (zeroed by the
 * caller) or NULL to switch the census off (the default). Env-substeps:
 *   [0] a hip / knee at its stop (contacts and limit rows through the general
 *       solver over scratch memory)
 *   [2] contact impulses outside the friction cone / pulling (an active-set
 *       solve, then projected Gauss-Seidel sweeps)
 *   [3] those of [2] an active-set solve answered (no sweep; since round 5)
 * wavefront-substeps (what the paths cost) that took, for at least one of their
 * eight envs, [4] the joint-stop path, [5] the sweeps. Sweeps run by the
 * env-substeps of [2]: [6] their sum, [7] the largest count, [1] how many
 * stopped at the iteration cap. Words [8 .. 71]: histogram
 * over the wavefront-substeps of [5] of the LARGEST sweep count among the
 * wavefront's envs (bin 63: 63 or more) -- what a launch waits for, since a
 * wavefront leaves the sweeps with its slowest env. Diagnostics only: no entry
 * point of the reference corresponds to it, and its atomics (up to five per
 * wavefront and substep on a rare path) are not free: time without it. */
#define UPKIE_CENSUS_WORDS 72
int upkie_sim_set_census(UpkieSim* sim, uint32_t* counters);

/* Optional per-env domain randomisation buffers (device pointers, may be
 * NULL): body_inertials[UPKIE_NB * UPKIE_INERTIAL_WORDS][B] replaces mass,
 * centre of mass and inertia of every composite body of every env (filled by
 * upkie_sim_sample_body_inertials; pybullet_backend.py:571-601); ext_force[3][B]
 * is a world-frame force applied at point `ext_point` of the trunk, re-applied
 * every substep until overwritten (pybullet_backend.py:603-658). */
int upkie_sim_set_randomization(UpkieSim* sim, const float* body_inertials,
                                const float* ext_force,
                                const double ext_point[3]);

/* External forces on any link, PyBulletBackend.set_external_forces /
 * __apply_external_forces (pybullet_backend.py:603-658): up to
 * UPKIE_MAX_EXTERNAL_FORCES forces act at the same time, each on one composite
 * body (0 trunk, 1-3 left thigh / calf / wheel, 4-6 right) at `point` given in
 * that body's frame (Bullet applies the force at the link's centre of mass),
 * expressed in the world frame (pybullet.WORLD_FRAME) or, with `local`, in the
 * body frame (pybullet.LINK_FRAME). forces[count][3][B] is a device buffer
 * read at every substep until replaced; NULL or count = 0 removes all forces.
 * Replaces whatever upkie_sim_set_randomization installed as ext_force. */
#define UPKIE_MAX_EXTERNAL_FORCES 16 /* one slot per link: upkie_description's Upkie has 15 */
typedef struct UpkieExternalForces {
  int32_t count;
  int32_t body[UPKIE_MAX_EXTERNAL_FORCES];
  int32_t local[UPKIE_MAX_EXTERNAL_FORCES];
  int32_t reserved0;
  double point[UPKIE_MAX_EXTERNAL_FORCES][3];
} UpkieExternalForces;

int upkie_sim_set_external_forces(UpkieSim* sim, const float* forces,
                                  const UpkieExternalForces* slots);

/* PyBulletBackend.randomize_inertias (pybullet_backend.py:571-601) for every
 * env: one epsilon ~ U(-v, v) per URDF link and env scales that link's mass
 * and inertia by (1 + epsilon); the links of each composite body are then
 * fused again (mass, centre of mass, inertia about it) into
 * body_inertials[UPKIE_NB * UPKIE_INERTIAL_WORDS][B], row 10 * body + word.
 * link_scale (may be NULL) receives the factors, [UPKIE_MAX_LINKS][B]. */
int upkie_sim_sample_body_inertials(UpkieSim* sim, float* body_inertials,
                                    float* link_scale,
                                    double inertia_variation, void* stream);

/* Push domain randomisation (BASELINE.json configs[4] "push-domain-randomisation";
 * the reference applies pushes through PyBulletBackend.set_external_forces,
 * pybullet_backend.py:603-658, with forces the user script draws:
 * examples/pybullet/apply_external_forces.py:37-43): push number `push_index`
 * of every env, a world-frame force with norm ~ U(0, max_norm) and a uniformly
 * random horizontal direction, drawn on the device from the Philox stream
 * keyed by (seed, global env id, push_index) into force[3][B] -- the buffer
 * upkie_sim_set_randomization / upkie_sim_set_external_forces read at every
 * substep. Zero the buffer to end the push. */
int upkie_sim_sample_pushes(UpkieSim* sim, float* force, uint32_t push_index,
                            double max_norm, void* stream);

/* ---- Episode events (random pushes, per-episode inertias) ----------------
 * The two perturbations a balancing policy is trained with, decided on the
 * device between two env steps, in ONE launch per env step
 * (csrc/episode_events.hpp), so that they can live inside a captured rollout:
 * pushes that start at random per env and are held a random number of steps
 * (what a RandomPush-style wrapper around the reference's
 * set_external_forces does, pybullet_backend.py:603-658), and link inertias
 * drawn again for every episode (randomize_inertias, :571-601, once per reset
 * of the reference's backend). The step kernels are not involved: `force` is
 * the [1][3][N] buffer upkie_sim_set_external_forces installed and
 * `body_inertials` the records upkie_sim_set_randomization installed; the
 * caller installs both once. State, device buffers of N = the handle's
 * num_envs words each, zero before the first call:
 *   calls uint32: calls so far;  remaining int32: steps the current force is
 *   still held, the coming one included;  pushes uint32: pushes started so
 *   far;  episodes uint32: episodes ended so far.
 * upkie_sim_episode_events_step, per env n, in this order:
 *   1. r = Philox4x32-10, counter (global env id lo, hi, calls[n],
 *      STREAM_EVENTS << 24 | 0) with STREAM_EVENTS = 6, key = the handle's
 *      seed; calls[n] += 1. Every env, every call: an env's draws depend
 *      neither on the batch, nor on the sharding, nor on other envs.
 *   2. if terminated[n] | truncated[n] (bytes; either may be NULL: 0):
 *      episodes[n] += 1, remaining[n] = 0 (a push does not outlive its
 *      episode) and, with inertia_variation > 0, the env's link factors are
 *      drawn as upkie_sim_sample_body_inertials draws them but with counter
 *      word 2 = episodes[n] (0 there), fused into the env's
 *      UPKIE_NB * UPKIE_INERTIAL_WORDS words of body_inertials and written to
 *      its column of link_scale [UPKIE_MAX_LINKS][N]. Other envs' words are
 *      not written.
 *   3. if remaining[n] > 0: remaining[n] -= 1.
 *   4. if remaining[n] == 0 the coming step is free: a push starts iff
 *      (r[0] >> 8) < llround(push_prob * 2^24). At a start, with
 *      k = pushes[n], the force is push number k of env n as
 *      upkie_sim_sample_pushes(push_index = k) defines it, but for its norm
 *      fma(push_norm_max - push_norm_min, u0, push_norm_min) (float32;
 *      push_norm_min = 0: the same value); pushes[n] += 1; remaining[n] =
 *      push_steps_min + (r[3] >> 8) % (push_steps_max - push_steps_min + 1).
 *      Without a start the three force words are +0.
 *   5. otherwise (a force is held) the force words are not written.
 * upkie_sim_episode_events_reset, for the envs with mask[n] != 0 (all when
 * mask is NULL): the four counters and the force back to 0 and, with
 * inertia_variation > 0, the records and factors of episode 0, which are
 * upkie_sim_sample_body_inertials'.
 * Refused with UPKIE_ERR_INVALID_ARGUMENT before anything else, with or
 * without a device: push_prob outside [0, 1], norms that are not finite with
 * 0 <= min <= max, steps outside 1 <= min <= max <= 65535, inertia_variation
 * outside [0, 1), push_prob == 0 with inertia_variation == 0 (nothing to do),
 * a NULL handle or state buffer, body_inertials / link_scale not given
 * exactly when inertia_variation > 0. No allocation, no host synchronisation,
 * no host argument that changes between calls: a step can be captured in a
 * hipGraph; the handle's seed and env_id_offset are read when the launch is
 * recorded. */
typedef struct UpkieEpisodeEvents {
  double push_prob;         /* per free env step */
  double push_norm_min;     /* N */
  double push_norm_max;
  double inertia_variation; /* 0: the records are left alone */
  int32_t push_steps_min;   /* env steps a push is held */
  int32_t push_steps_max;
} UpkieEpisodeEvents;

int upkie_sim_episode_events_step(UpkieSim* sim, const UpkieEpisodeEvents* params, const uint8_t* terminated,
                                  const uint8_t* truncated, uint32_t* calls, int32_t* remaining, uint32_t* pushes,
                                  uint32_t* episodes, float* force, float* body_inertials, float* link_scale,
                                  void* stream);

int upkie_sim_episode_events_reset(UpkieSim* sim, const UpkieEpisodeEvents* params, const uint8_t* mask, uint32_t* calls,
                                   int32_t* remaining, uint32_t* pushes, uint32_t* episodes, float* force,
                                   float* body_inertials, float* link_scale, void* stream);

/* ---- Push curriculum (per-env difficulty levels, live push settings) ------
 * The episode events with two additions, in the launch the stage already has:
 * the push settings are a device block read at every call, not launch
 * arguments, so whoever rewrites the block (a device copy) is followed by a
 * captured step at its next replay; and every env carries a difficulty level
 * that rises when its episode survives to the time limit under pushes, falls
 * when the robot falls, and scales the norm range of that env's pushes
 * (legged_gym's terrain levels, applied to pushes). A level depends on its own
 * env's history alone: no reduction, no host decision, nothing to exchange
 * between the ranks of a sharded run. upkie_sim_episode_events_step / _reset
 * above are not changed by any of this.
 * State beyond the four counters, N words each:
 *   level uint32: the env's difficulty level;  episode_pushes uint32: push
 *   starts in the current episode;  difficulty float: the fraction the coming
 *   step's pushes are scaled by, written for every env at every call.
 * settings: UPKIE_EVENTS_SETTINGS_WORDS 32-bit device words, in this order:
 *   threshold uint32 (llround(push_prob * 2^24)), norm_min, norm_max float,
 *   steps_min, steps_span uint32 (steps_span = steps_max - steps_min + 1; 0 is
 *   read as 1), levels = L uint32 (0..UPKIE_EVENTS_LEVELS_MAX), up, down
 *   uint32 (0..L), min_pushes uint32.
 * inertia_variation stays a host argument: it decides which buffers exist.
 * upkie_sim_episode_events_step_levels, per env n, with l = min(level[n], L)
 * (a level read above L is taken as L):
 *   1. as step 1 above: the same stream, counter and key. A level never
 *      changes which random words an env draws.
 *   2. if the episode ended, before anything else of step 2: if terminated[n]
 *      (it wins when both flags are set): l -= min(l, down); otherwise (the
 *      episode was truncated) if episode_pushes[n] >= min_pushes:
 *      l = min(l + up, L). Then episode_pushes[n] = 0, then step 2 above.
 *   3. as above.
 *   4. as above, with the block's threshold, steps_min and steps_span, and at
 *      a push start: hi = norm_max when l >= L (which includes L = 0),
 *      otherwise hi = fma(norm_max - norm_min, (float)l / (float)L, norm_min)
 *      in float32; the norm is fma(hi - norm_min, u0, norm_min): with
 *      hi = norm_max the expression of step 4 above, to the bit;
 *      episode_pushes[n] += 1. A push that starts on the call that ended an
 *      episode uses the new level.
 *   5. as above. Then level[n] = l, and difficulty[n] = 1 when l >= L, else
 *      (float)l / (float)L (IEEE division).
 * upkie_sim_episode_events_reset_levels: the reset above, then, for the same
 * envs, level[n] = start_level, episode_pushes[n] = 0 and difficulty[n] that
 * of start_level.
 * upkie_sim_episode_events_level_counts: counts uint32
 * [UPKIE_EVENTS_LEVELS_MAX + 1], zeroed by the call (a memset node in front of
 * the launch), then counts[l] = the number of envs with level[n] == l (a level
 * above UPKIE_EVENTS_LEVELS_MAX counts at UPKIE_EVENTS_LEVELS_MAX). Integer
 * sums only: the order of the additions cannot change a bit. Any N.
 * Refused with UPKIE_ERR_INVALID_ARGUMENT before anything else, with or
 * without a device: a NULL handle, state buffer or settings, start_level above
 * UPKIE_EVENTS_LEVELS_MAX, inertia_variation outside [0, 1), body_inertials /
 * link_scale not given exactly when inertia_variation > 0. (The block's words
 * are device words: upkie_amd.events checks them before it writes them.) No
 * allocation, no host synchronisation, no host argument that changes between
 * calls: a step can be captured in a hipGraph. */
#define UPKIE_EVENTS_SETTINGS_WORDS 9
#define UPKIE_EVENTS_LEVELS_MAX 255

int upkie_sim_episode_events_step_levels(UpkieSim* sim, double inertia_variation, const uint32_t* settings,
                                         const uint8_t* terminated, const uint8_t* truncated, uint32_t* calls,
                                         int32_t* remaining, uint32_t* pushes, uint32_t* episodes, uint32_t* level,
                                         uint32_t* episode_pushes, float* difficulty, float* force, float* body_inertials,
                                         float* link_scale, void* stream);

int upkie_sim_episode_events_reset_levels(UpkieSim* sim, double inertia_variation, const uint32_t* settings,
                                          uint32_t start_level, const uint8_t* mask, uint32_t* calls, int32_t* remaining,
                                          uint32_t* pushes, uint32_t* episodes, uint32_t* level, uint32_t* episode_pushes,
                                          float* difficulty, float* force, float* body_inertials, float* link_scale,
                                          void* stream);

int upkie_sim_episode_events_level_counts(UpkieSim* sim, const uint32_t* level, uint32_t* counts, void* stream);

/* ---- Task targets (goals in the observation, a curriculum) ----------------
 * The goal an env is asked to reach -- a ground and a yaw velocity, say --
 * drawn per env on the device, held a random number of env steps, drawn again
 * when the hold or the episode ends, and appended to the observation row the
 * policy, the reward terms and the critic read: legged_gym's "commands" and
 * "command curriculum" (csrc/task_targets.hpp), ONE launch per env step, so
 * that it can live inside a captured rollout. ("Command" is the shaped action
 * here, so the goal is the TARGET.) D = obs_dim words of observation,
 * G = num_targets words of target, 1 <= G <= UPKIE_TASK_TARGETS_MAX,
 * D + G <= 256; N = the handle's num_envs. Device buffers:
 *   calls uint32 [N]: draws so far;  remaining int32 [N]: steps the current
 *   target is still held, the coming one included;  target float [G][N];
 *   limits float [G][2]: (low, high) of every word, read at every draw -- a
 *   device block, not a launch argument: whoever rewrites it (a device copy,
 *   the curriculum below) is followed by a captured step at its next replay;
 *   observation, final_observation float [N][D + G].
 * upkie_sim_task_targets_step, per env n, in this order:
 *   1. r = Philox4x32-10, counter (global env id lo, hi, calls[n],
 *      STREAM_TARGETS << 24 | 0) with STREAM_TARGETS = 7, key = the handle's
 *      seed; calls[n] += 1. Every env, every call: an env's draws depend
 *      neither on the batch, nor on the sharding, nor on other envs.
 *   2. final_observation[n], for EVERY env: final_obs[n] where
 *      terminated[n] | truncated[n] (bytes; either may be NULL: 0; next_obs[n]
 *      when final_obs is NULL) and next_obs[n] elsewhere, followed by the OLD
 *      target[:][n]: the step's outcome under the target the policy was given.
 *   3. an ended episode: remaining[n] = 0; otherwise if remaining[n] > 0:
 *      remaining[n] -= 1.
 *   4. if remaining[n] == 0, a new target, "the draw" of (n, c = the calls[n]
 *      that step 1 read, r):
 *      remaining[n] = resample_steps_min + (r[3] >> 8) % (resample_steps_max -
 *      resample_steps_min + 1); if (r[0] >> 8) < llround(stand_prob * 2^24)
 *      every word is +0; otherwise word g is fma(limits[g][1] - limits[g][0],
 *      u, limits[g][0]) in float32 with u = (w >> 8) / 2^24 and w word g % 4 of
 *      the Philox block of counter (id lo, hi, c, STREAM_TARGETS << 24 |
 *      1 + g / 4); a word with |x| < deadband[g] becomes +0.
 *   5. observation[n] = next_obs[n] followed by the current target[:][n].
 * upkie_sim_task_targets_reset, for the envs with mask[n] != 0 (all when mask
 * is NULL): the draw of (n, c = 0, r of counter word 2 = 0), calls[n] = 1 (the
 * draw was the env's call 0: no step draws from its blocks again), then
 * observation[n] = obs[n] followed by the target. final_observation and the
 * other envs' words are not written.
 * upkie_sim_task_targets_curriculum (one launch per training iteration,
 * outside the rollout): score double [N] and finished int32 [N] are an
 * episode score per env and the count of episodes it has finished (the reward
 * terms' term_last[k] and finished); seen int32 [N], zero at first. Over the
 * envs with finished[n] != seen[n]: S = sum of score[n], M = their count,
 * seen[n] = finished[n]. If M > 0 and S > threshold * M (fp64, no division),
 * for every g: limits[g][0] = max(limits[g][0] - step[g], limit[g][0]) and
 * limits[g][1] = min(limits[g][1] + step[g], limit[g][1]) in float32;
 * otherwise limits is not written. step [G] and limit [G][2] are HOST arrays.
 * The sum is taken in a fixed order (per block of 2048 envs: thread t of 256
 * adds envs t, t + 256, ... in that order, then a halving tree; the blocks'
 * partials in block order), in fp64, without float atomics: the same bits
 * every call. workspace: upkie_sim_task_targets_workspace_bytes bytes (a
 * function of num_envs alone; negative: refused), zero before the first call.
 * Refused with UPKIE_ERR_INVALID_ARGUMENT before anything else, with or
 * without a device: num_targets outside 1..UPKIE_TASK_TARGETS_MAX, obs_dim < 1
 * or obs_dim + num_targets > 256, stand_prob outside [0, 1], resample steps
 * outside 1 <= min <= max <= 65535, a deadband that is negative or not finite,
 * a curriculum step that is negative or not finite, a curriculum limit that
 * is not finite with low <= high, a threshold that is NaN, a NULL handle,
 * state buffer, limits or next_obs. (The ranges themselves are device words:
 * upkie_amd.targets checks them, finite with low <= high, before it writes
 * them.) No allocation, no host synchronisation, no host argument that
 * changes between calls: a step can be captured in a hipGraph; the handle's
 * seed and env_id_offset are read when the launch is recorded. */
#define UPKIE_TASK_TARGETS_MAX 8

typedef struct UpkieTaskTargets {
  double stand_prob; /* per draw: every word +0 */
  double deadband[UPKIE_TASK_TARGETS_MAX];
  int32_t obs_dim;     /* D */
  int32_t num_targets; /* G */
  int32_t resample_steps_min; /* env steps a target is held */
  int32_t resample_steps_max;
} UpkieTaskTargets;

int upkie_sim_task_targets_step(UpkieSim* sim, const UpkieTaskTargets* params, const float* next_obs, const float* final_obs,
                                const uint8_t* terminated, const uint8_t* truncated, const float* limits, uint32_t* calls,
                                int32_t* remaining, float* target, float* observation, float* final_observation,
                                void* stream);

int upkie_sim_task_targets_reset(UpkieSim* sim, const UpkieTaskTargets* params, const float* obs, const uint8_t* mask,
                                 const float* limits, uint32_t* calls, int32_t* remaining, float* target,
                                 float* observation, void* stream);

int64_t upkie_sim_task_targets_workspace_bytes(int32_t num_envs);

int upkie_sim_task_targets_curriculum(UpkieSim* sim, int32_t num_targets, double threshold, const float* step,
                                      const float* limit, const double* score, const int32_t* finished, int32_t* seen,
                                      float* limits, void* workspace, void* stream);

/* Diagnostic: the projected Gauss-Seidel sweeps the step kernels run when the
 * direct contact solution leaves its friction cone (what Bullet's
 * btMultiBodyConstraintSolver iterates inside pybullet.stepSimulation(),
 * pybullet_backend.py:306), on caller-provided 6 x 6 systems of the two tires
 * (rows: normal, rolling, lateral of the left tire, then of the right one), one
 * system per lane, with this handle's friction coefficient, tolerance and
 * iteration cap: A[n][21] packed lower by rows with the CFM on the diagonal,
 * rhs[n][6], lam[n][6] (in: warm start, out: impulses), both_tires[n] (0: one
 * tire is off the floor, its rows are identity rows with zero right-hand
 * sides and no coupling; informative since round 4: every system runs the
 * same loop, which such rows pass through unchanged), sweeps[n] (may be NULL)
 * receives the sweeps each system ran. Device pointers. */
int upkie_sim_contact_sweeps(UpkieSim* sim, int32_t num_systems, const float* A,
                             const float* rhs, float* lam,
                             const uint8_t* both_tires, int32_t* sweeps,
                             void* stream);

/* Reset the envs whose mask byte is non-zero (all when mask is NULL):
 * sample the initial state in the reference's draw order (robot_state.py:
 * 182-187), zero joint velocities, run the one extra torque-free physics
 * substep (pybullet_backend.py:220-232) and seed the Gyropod filter state
 * (upkie_gyropod.py:236-240). obs6 (may be NULL) receives the Gyropod
 * observation [B][6]. */
int upkie_sim_reset(UpkieSim* sim, float* state, const uint8_t* mask,
                    float* obs6, void* stream);

/* One env.step() of UpkiePendulum (upkie_pendulum.py:124-142) for every env:
 * act[B] ground velocity -> obs[B][4] = [pitch, position, pitch rate, velocity],
 * reward[B] = 0, terminated[B], truncated[B] = 0. */
int upkie_sim_step_pendulum(UpkieSim* sim, float* state, const float* act,
                            float* obs, float* reward, uint8_t* terminated,
                            uint8_t* truncated, void* stream);

/* Same step with the README's linear-feedback agent evaluated on-device from
 * the previous observation held in `obs` (in/out). */
int upkie_sim_step_pendulum_agent(UpkieSim* sim, float* state, float* obs,
                                  float* reward, uint8_t* terminated,
                                  uint8_t* truncated, void* stream);

/* Packed-record variants for rollout collection across GPUs: instead of four
 * output arrays each env gets one 32-byte record records[B][8] =
 * [obs(4) | reward, terminated, truncated, 0] (two 16-byte stores per lane),
 * which is what one RCCL gather per step ships to rank 0. The agent variant
 * reads the previous observation from the record. */
int upkie_sim_step_pendulum_packed(UpkieSim* sim, float* state,
                                   const float* act, float* records,
                                   void* stream);
int upkie_sim_step_pendulum_agent_packed(UpkieSim* sim, float* state,
                                         float* records, void* stream);
/* Double-buffered form: the agent reads the previous observation from
 * prev_records (a different buffer) so that a gather of prev_records can still
 * be in flight while this step runs. */
int upkie_sim_step_pendulum_agent_records(UpkieSim* sim, float* state,
                                          const float* prev_records,
                                          float* records, void* stream);

/* num_steps consecutive env.step() of the same fused-agent Pendulum env, i.e.
 * num_steps calls of upkie_sim_step_pendulum_agent_records with
 * records[k - 1] as the previous records of step k (prev_records for k = 0):
 * records [num_steps][B][8]. Up to 32768 envs this is ONE launch in which the
 * state stays in registers from step to step (the agent needs nothing from the
 * host in between); results are bit-identical to the step-by-step calls. */
int upkie_sim_step_pendulum_agent_rollout(UpkieSim* sim, float* state,
                                          const float* prev_records,
                                          float* records, int32_t num_steps,
                                          void* stream);

/* One env.step() of UpkieGyropod (upkie_gyropod.py:354-392):
 * act[B][2] -> obs[B][6]. Buffers of row-major observations, actions and
 * records are read and written with 8- and 16-byte accesses: keep them
 * 16-byte aligned (any allocator's default). */
int upkie_sim_step_gyropod(UpkieSim* sim, float* state, const float* act,
                           float* obs, float* reward, uint8_t* terminated,
                           uint8_t* truncated, void* stream);

/* One env.step() of UpkieBaseVelocity (upkie_base_velocity.py:164-202) after
 * upkie_mpc_step_env(): act[B][2] = [linear velocity, yaw velocity]; the
 * ground velocity commanded to the Gyropod layer is commanded_velocity[B]
 * (the MPC balancer's output). obs[B][3] = dead-reckoned [x, y, yaw]. Also
 * writes what the balancer reads at the next step: mpc_x0[B][4] = [ground
 * position, pitch, ground velocity, pitch rate], mpc_contact[B]. */
int upkie_sim_step_base_velocity(UpkieSim* sim, float* state, const float* act,
                                 const float* commanded_velocity, float* obs,
                                 float* mpc_x0, uint8_t* mpc_contact,
                                 float* reward, uint8_t* terminated,
                                 uint8_t* truncated, void* stream);

/* The same step with MPCBalancer.step() in front of it in ONE launch
 * (upkie_base_velocity.py:164-202 as a whole): equivalent to
 * upkie_mpc_step_env(mpc, workspace, mpc_x0, act, mpc_contact, <done words of
 * the state when autoreset is on>, dt, commanded_velocity) followed by
 * upkie_sim_step_base_velocity(...), bit for bit. One kernel when envs are
 * mapped two lanes each and the horizon fits one 16-row tile (the wavefront
 * that steps 32 envs first solves their condensed QPs on the matrix cores and
 * hands the velocities over through LDS); the two launches otherwise. */
struct UpkieMpc;
int upkie_sim_step_base_velocity_mpc(UpkieSim* sim, struct UpkieMpc* mpc, float* state, float* workspace,
                                     const float* act, float* commanded_velocity, float* obs,
                                     float* mpc_x0, uint8_t* mpc_contact, float* reward,
                                     uint8_t* terminated, uint8_t* truncated, void* stream);

/* One env.step() of UpkieServos (upkie_servos.py:316-344 + upkie_env.py:
 * 196-242): act[B][6][6] in ACTION_KEYS order (position, velocity,
 * feedforward_torque, kp_scale, kd_scale, maximum_torque) -> obs[B][6][5]
 * (position, velocity, torque, temperature, voltage). */
int upkie_sim_step_servos(UpkieSim* sim, float* state, const float* act,
                          float* obs, float* reward, uint8_t* terminated,
                          uint8_t* truncated, void* stream);

/* On-device servo-level policy for UpkieServos: ONE small launch that writes the
 * action buffer act[B][6][6] of the next upkie_sim_step_servos from the state,
 * so that a servo-level agent needs no host round trip (BASELINE.json
 * configs[4]). The law is examples/pybullet/torque_balancing.py:15-37 with
 * room for the README's velocity feedback: every joint j starts from
 * `action[j]` (ACTION_KEYS order) and gets
 *   feedforward_torque += pitch_to_torque[j] * pitch
 *   velocity           += clip(pitch_to_velocity[j] * pitch + position_to_velocity[j] * p + velocity_to_velocity[j] * pdot,
 *                               +-velocity_feedback_clip[j])        (no clipping where velocity_feedback_clip[j] <= 0)
 * with pitch = base_orientation.pitch of the spine observation and p, pdot the
 * ground position / velocity of upkie_gyropod.py:186-214 (wheel odometry).
 * Envs with |pitch| > fall_pitch get their UPKIE_S_DONE word set: with
 * UPKIE_AUTORESET_NEXT_STEP the step that follows re-initialises them (what the
 * example's `if terminated or truncated: env.reset()` does); fall_pitch <= 0
 * switches that off. */
typedef struct UpkieServoPolicy {
  float action[UPKIE_NJ][6];
  float pitch_to_torque[UPKIE_NJ];
  float pitch_to_velocity[UPKIE_NJ];
  float position_to_velocity[UPKIE_NJ];
  float velocity_to_velocity[UPKIE_NJ];
  float velocity_feedback_clip[UPKIE_NJ];
  float fall_pitch;
} UpkieServoPolicy;
int upkie_sim_servo_policy(UpkieSim* sim, float* state, const UpkieServoPolicy* policy, float* act, void* stream);
/* upkie_sim_servo_policy + upkie_sim_step_servos as one call: on the
 * eight-lanes-per-env mapping (batches up to 8192 envs) the policy is evaluated
 * inside the step's launch, each joint lane computing its own command from the
 * state the step starts from, and `act` is left untouched; on the other
 * mappings the two launches run one behind the other through `act` ([B][6][6],
 * caller's scratch). Same results up to the rounding of the feedback sum. */
int upkie_sim_step_servos_policy(UpkieSim* sim, float* state, const UpkieServoPolicy* policy, float* act, float* obs, float* reward,
                                 uint8_t* terminated, uint8_t* truncated, void* stream);

/* Full spine observation (pybullet_backend.py:313-490), materialised lazily.
 * Any pointer may be NULL. */
typedef struct UpkieSpineObservation {
  float* pitch;                  /* [B]                                     */
  float* angular_velocity;       /* [B][3] base in base                     */
  float* linear_velocity;        /* [B][3] base in world                    */
  float* rotation_base_to_world; /* [B][9] row-major                        */
  uint8_t* floor_contact;        /* [B]                                     */
  float* imu_orientation;        /* [B][4] w x y z, IMU in ARS              */
  float* imu_angular_velocity;   /* [B][3]                                  */
  float* imu_linear_acceleration;     /* [B][3]                             */
  float* imu_raw_linear_acceleration; /* [B][3]                             */
  float* servo;                  /* [B][6][5]                               */
  float* wheel_odometry;         /* [B][2] position, velocity               */
} UpkieSpineObservation;

/* gymnasium.vector AutoresetMode.SAME_STEP: the step that ends an episode
 * also returns the first observation of the next one, the terminal observation
 * going to info["final_obs"]. Call after a step made with
 * UPKIE_AUTORESET_DISABLED: every env whose DONE word is set (by the step when
 * the robot fell, or by the caller for a time limit: row UPKIE_S_DONE of the
 * state) is re-initialised exactly as upkie_sim_reset does it and its row of
 * `obs` (the buffer the step wrote, in that step's layout) replaced by the
 * reset observation; `final_obs` (same layout, may be NULL; records: [B][4])
 * receives the step's observation of EVERY env first. Reward and flags of the
 * terminal step stay; envs that are not done are otherwise untouched. One
 * launch. */
enum UpkieObservationLayout {
  UPKIE_OBSERVATION_PENDULUM = 1,         /* [B][4], upkie_sim_step_pendulum            */
  UPKIE_OBSERVATION_PENDULUM_RECORDS = 2, /* [B][8] records, ..._step_pendulum_packed   */
  UPKIE_OBSERVATION_GYROPOD = 3,          /* [B][6], upkie_sim_step_gyropod             */
  UPKIE_OBSERVATION_SERVOS = 4            /* [B][6][5], upkie_sim_step_servos           */
};
int upkie_sim_autoreset_done(UpkieSim* sim, int observation, float* state,
                             float* obs, float* final_obs, void* stream);

/* Output buffers must be 16-byte aligned (the rows of 64 consecutive envs are
 * streamed out with 16-byte stores).
 * update_imu != 0 advances the finite-difference accelerometer memory the
 * way one get_spine_observation() call does (pybullet_backend.py:405-408). */
int upkie_sim_observe(UpkieSim* sim, float* state,
                      const UpkieSpineObservation* out, int update_imu,
                      void* stream);

/* Replaces PyBulletBackend.get_contact_points (upkie/envs/backends/
 * pybullet_backend.py:660-716) for the whole batch. The only links that can
 * touch the floor are the two tires, with at most one contact point each:
 *   out [B][2][UPKIE_CONTACT_POINT_WORDS] = per tire (0 "left_wheel_tire",
 *   1 "right_wheel_tire") {exists (0/1), position_contact_in_world (3),
 *   force_in_world (3) = normal + both friction forces in N, 0}.
 * The forces are those of the contact solve of one simulator substep from the
 * current state under the last commanded torques (Bullet reports the last
 * solved substep; the two differ by one 1 ms substep of motion). `state` is
 * only read. On a handle under the Bullet-like contact model
 * (upkie_sim_set_contact_manifold) the query solves THAT model, on a copy of
 * the env's manifold: per tire its (first) cached point and the force the
 * impulses of its points sum to. */
#define UPKIE_CONTACT_POINT_WORDS 8
int upkie_sim_contact_points(UpkieSim* sim, const float* state, float* out, void* stream);

/* ---- MPC balancer (upkie/controllers/mpc_balancer.py:168-312) ---------- */
typedef struct UpkieMpcConfig {
  int32_t num_envs;
  int32_t nb_timesteps;  /* N, 50 by default in the reference               */
  int32_t admm_iterations;
  int32_t reserved0;
  double sampling_period;         /* 0.02 */
  double leg_length;              /* 0.58 */
  double max_ground_accel;        /* 10.0 */
  double max_ground_velocity;     /* 3.0  */
  double fall_pitch;              /* 1.0  */
  double stage_input_cost_weight; /* 1e-3 */
  double stage_state_cost_weight; /* 1e-3 */
  double terminal_cost_weight;    /* 1.0  */
  double admm_rho;
  double admm_relaxation; /* over-relaxation alpha of the ADMM iteration (Boyd et al. 2011, section 3.4.3; OSQP's
                             default is 1.6): x^ = alpha x + (1 - alpha) z replaces x in the z- and y-updates.
                             1.0 (or 0: unset) = the plain iteration; 1.5 by default: same fixed point, and at the
                             reference's N = 50 an order of magnitude closer to it after the same 30 iterations */
} UpkieMpcConfig;

typedef struct UpkieMpc UpkieMpc;

int upkie_mpc_create(const UpkieMpcConfig* config, UpkieMpc** out);
int upkie_mpc_destroy(UpkieMpc* mpc);
const char* upkie_mpc_last_error(const UpkieMpc* mpc);
/* Bytes of the warm-start workspace [2 N][B] the caller allocates. */
int64_t upkie_mpc_workspace_bytes(const UpkieMpc* mpc);
/* MPCBalancer.reset (mpc_balancer.py:228-235) for masked envs. */
int upkie_mpc_reset(UpkieMpc* mpc, float* workspace, float* commanded_velocity,
                    const uint8_t* mask, void* stream);
/* MPCBalancer.step (mpc_balancer.py:237-312) for every env. x0[B][4] =
 * [ground position, pitch, ground velocity, pitch rate]; contact[B] floor
 * contact flags; commanded_velocity[B] in/out; first_input[B] (may be NULL)
 * receives plan.first_input.
 * Arithmetic: fixed-iteration ADMM on the condensed QP, its dense product on the
 * matrix cores: v_mfma_f32_16x16x32_f16 on two fp16 terms per operand with fp32
 * accumulation, the constant part of the product (Minv q) computed once per step
 * from fp64 host products (csrc/mpc.hpp: first input within 5e-4 m/s2 of the fp64
 * oracle's at N = 16 .. 64). A solve whose iterates leave fp16's range (a finite but
 * absurd target or state: |64 rho (2 z - w)| > 65504), or whose constant part Minv q
 * exceeds 1e5 in any element (e.g. a target velocity of 1e30),
 * is discarded as a whole: zero warm start, first_input 0, the commanded velocity
 * decays as for a fallen robot; nothing non-finite is ever stored (non-finite TARGETS
 * are replaced by 0 up front, see "Non-finite commands and states").
 * The environment variable UPKIE_MPC_FP32=1, read at the
 * first step of the process, selects the fp32 MFMA kernels of earlier rounds for this
 * entry point (A/B). */
int upkie_mpc_step(UpkieMpc* mpc, float* workspace, const float* x0,
                   const float* target_velocity, const uint8_t* contact,
                   double dt, float* commanded_velocity, float* first_input,
                   void* stream);

/* MPCBalancer.step as the first half of a fused UpkieBaseVelocity env.step():
 * the target velocity of env e is act[2 e] (act is the env's [B][2] action),
 * and envs whose `done` word (row UPKIE_S_DONE of the state, may be NULL) is
 * set get MPCBalancer.reset() instead of a solve, because the env step that
 * follows resets them (NEXT_STEP autoreset). */
int upkie_mpc_step_env(UpkieMpc* mpc, float* workspace, const float* x0,
                       const float* act, const uint8_t* contact,
                       const float* done, double dt, float* commanded_velocity,
                       void* stream);

/* ---- Spine observer pipeline ---------------------
 * Device restatement of the observers the real spine runs after every cycle
 * (spines/common/observers.h:22-42): BaseOrientation
 * (upkie/cpp/observers/BaseOrientation.{h,cpp}), FloorContact
 * (FloorContact.cpp:37-104) with its two WheelContact estimators
 * (WheelContact.cpp:19-48) and the velocity-integrating WheelOdometry
 * (WheelOdometry.cpp:16-54), in that order, for every env of a batch. Sim
 * observations then carry what an agent sees on the real robot. */
typedef struct UpkieObserverConfig {
  int32_t num_envs;
  int32_t reserved0;
  double dt; /* spine period, FloorContact::Parameters::dt / WheelOdometry::Parameters::dt */
  double upper_leg_torque_threshold; /* 10.0  (FloorContact.h:82)            */
  double wheel_cutoff_period;        /* 0.2   (spine_backend.py:93); < 1e-6 =
                                        "not configured": wheel observers idle
                                        (WheelContact.cpp:21-24)             */
  double liftoff_inertia;            /* 0.001 */
  double min_touchdown_acceleration; /* 2.0   */
  double min_touchdown_torque;       /* 0.015 */
  double touchdown_inertia;          /* 0.004 */
  double signed_radius[2];           /* left, right: +0.05, -0.05 (spine_backend.py:99-104) */
  double rotation_base_to_imu[9];    /* row-major, diag(-1, 1, -1) (BaseOrientation.h:161-162) */
  double rotation_ars_to_world[9];   /* row-major, diag(1, -1, -1) (BaseOrientation.h:163-164) */
} UpkieObserverConfig;

/* Observer memory, struct-of-arrays [UPKIE_OBSERVER_STATE_WORDS][B] fp32,
 * allocated by the caller. */
enum UpkieObserverStateWord {
  UPKIE_O_WHEEL = 0, /* 2 wheels x (velocity, abs_acceleration, abs_torque, inertia, contact) */
  UPKIE_O_UPPER_LEG_TORQUE = 10,
  UPKIE_O_CONTACT = 11,
  UPKIE_O_ODOMETRY_POSITION = 12,
  UPKIE_O_ODOMETRY_VELOCITY = 13,
  UPKIE_OBSERVER_STATE_WORDS = 16
};

/* What the observers read from the spine observation (device pointers, the
 * layouts of UpkieSpineObservation). imu_orientation == NULL skips
 * BaseOrientation (no "imu" key, BaseOrientation.cpp:17-19); cross_button
 * may be NULL. */
typedef struct UpkieObserverInput {
  const float* servo;                /* [B][6][5]                             */
  const float* imu_orientation;      /* [B][4] w x y z, IMU in ARS            */
  const float* imu_angular_velocity; /* [B][3]                                */
  const uint8_t* cross_button;       /* [B] joystick.cross_button             */
} UpkieObserverInput;

/* What they write (any pointer may be NULL). */
typedef struct UpkieObserverOutput {
  float* base_pitch;             /* [B]    base_orientation.pitch             */
  float* base_angular_velocity;  /* [B][3] base in base                       */
  float* rotation_base_to_world; /* [B][9] row-major                          */
  uint8_t* floor_contact;        /* [B]    floor_contact.contact              */
  float* upper_leg_torque;       /* [B]    floor_contact.upper_leg_torque     */
  float* wheel_contact;          /* [B][2][4] per wheel: abs_acceleration,
                                    abs_torque, contact (0/1), inertia
                                    (FloorContact.cpp:96-103)                 */
  float* wheel_odometry;         /* [B][2] position, velocity                 */
} UpkieObserverOutput;

typedef struct UpkieObservers UpkieObservers;

/* Fails with UPKIE_ERR_INVALID_ARGUMENT where the reference throws:
 * cutoff period <= 2 dt (FilterError, low_pass_filter.h:22-30) for the wheel
 * filters or for the 0.01 s upper-leg torque filter (FloorContact.cpp:87). */
int upkie_observers_create(const UpkieObserverConfig* config, UpkieObservers** out);
int upkie_observers_destroy(UpkieObservers* observers);
const char* upkie_observers_last_error(const UpkieObservers* observers);
int64_t upkie_observers_state_bytes(const UpkieObservers* observers);
/* Observer::reset for masked envs (all when mask is NULL): filters, contacts
 * and odometry back to zero (FloorContact.cpp:26-35, WheelOdometry.cpp:10-14). */
int upkie_observers_reset(UpkieObservers* observers, float* state, const uint8_t* mask, void* stream);
/* Run FloorContact / WheelContact / WheelOdometry INSIDE every env step, one
 * observer cycle per 1 ms physics substep: what the spine does under a slower
 * agent (Spine::simulate, Spine.cpp:119-141: nb_substeps cycles per action).
 * The spine period is the substep dt / nb_substeps (config->dt is ignored);
 * observer_state is the caller's [UPKIE_OBSERVER_STATE_WORDS][B] buffer, read
 * and written by the step kernels and cleared for envs that (auto)reset; its
 * words are the observers' outputs. NULL config or state detaches. */
int upkie_sim_attach_observers(UpkieSim* sim, const UpkieObserverConfig* config, float* observer_state);

/* One ObserverPipeline::run (read + write of the three observers). in->servo
 * == NULL: no "servo" block, only BaseOrientation runs (FloorContact.cpp:42-44). */
int upkie_observers_step(UpkieObservers* observers, float* state, const UpkieObserverInput* in,
                         const UpkieObserverOutput* out, void* stream);

/* A linear policy in one launch, for the loop `obs, ... = env.step(policy(obs))`
 * that the reference leaves to the agent (README.md:60-67: action = clamp(gains
 * . obs)): act[n][a] = clamp(sum_d obs[n][d] weights[d][a] + bias[a], -clip,
 * clip) for n < num_envs; bias may be NULL, clip <= 0 disables the clamp. obs
 * [num_envs][obs_dim], weights [obs_dim][act_dim], act [num_envs][act_dim],
 * contiguous fp32 device buffers. (As torch ops the same policy is two or
 * three launches of 2-5 us each behind a 14.5 us step.) */
int upkie_linear_policy(int32_t num_envs, int32_t obs_dim, int32_t act_dim, const float* obs,
                        const float* weights, const float* bias, double clip, float* act,
                        void* stream);

/* ---- MLP actor-critic policy (one launch per rollout step) ---------------
 * The policy side of a rollout step as one launch: what Stable-Baselines3's
 * MlpPolicy evaluates between two env steps (separate actor and critic towers,
 * one activation, a diagonal Gaussian with a state-independent log_std,
 * optionally VecNormalize statistics: frozen, or kept live in the packed
 * buffer by upkie_vecnorm_step's packed_stats), computed on fp32 MFMA
 * (csrc/policy_mlp.hpp). For each env n < num_envs:
 *   x        = clamp((obs - obs_mean) / obs_std, -clip_obs, clip_obs)
 *              (obs_std = sqrt(var + eps); x = obs when normalize == 0)
 *   mean     = actor(x)                      [act_dim]
 *   value    = critic(x)                     (scalar)
 *   action   = mean + exp(log_std) * z       (action = mean when deterministic)
 *   log_prob = sum_a -(action_a - mean_a)^2 / (2 sigma_a^2) - log_std_a - log(2 pi) / 2
 *              (SB3's DiagGaussianDistribution.log_prob of the UNCLIPPED action)
 *   env_action = clamp(action, action_low, action_high), per dimension.
 * A tower is 1-4 hidden layers of 1-256 units (critic_layers == 0: no critic)
 * and a linear head; 1 <= obs_dim <= 256, 1 <= act_dim <= 64.
 *
 * Sampling. z of action a of env n is normal a & 3 of Philox4x32-10 block
 *   counter = (n, calls[n], 0, (4 << 24) | (a >> 2)), key = (seed lo, seed hi),
 * where calls[n] is the env's uint32 call counter in device memory (read by the
 * launch, incremented by one after it; deterministic launches neither read nor
 * advance it, so no host argument changes between calls and the launch can be
 * captured in a hipGraph). The block's words r0..r3 give two Box-Muller pairs,
 *   u1 = ((r[2p] >> 8) + 1) / 2^24 in (0, 1] (never 0), u2 = (r[2p+1] >> 8) / 2^24,
 *   z[2p] = sqrt(-2 ln u1) cos(2 pi u2), z[2p+1] = sqrt(-2 ln u1) sin(2 pi u2).
 * (Tag 4 in the top byte of counter word 3 keeps these draws apart from the
 * step kernels' streams, tags 0-3.)
 *
 * Weights are read from one packed fp32 buffer of upkie_mlp_packed_words(shape)
 * words in MFMA fragment order (layout: csrc/policy_mlp.hpp;
 * upkie_amd/policies.py packs it from torch modules, on the device). */
#define UPKIE_MLP_MAX_LAYERS 4
enum UpkieMlpActivation { UPKIE_MLP_TANH = 0, UPKIE_MLP_RELU = 1 };
typedef struct {
  int32_t obs_dim;
  int32_t act_dim;
  int32_t activation; /* UpkieMlpActivation, for every hidden layer of both towers */
  int32_t actor_layers;
  int32_t actor_widths[UPKIE_MLP_MAX_LAYERS];
  int32_t critic_layers; /* 0: no critic */
  int32_t critic_widths[UPKIE_MLP_MAX_LAYERS];
  int32_t normalize; /* 1: observation normalisation with the packed obs_mean / obs_std */
  float clip_obs;    /* VecNormalize's clip_obs (> 0 when normalize) */
  int32_t critic_obs_dim; /* 0: the critic reads obs; 1-256: a row of its own (asymmetric, needs critic_layers >= 1) */
} UpkieMlpShape;

/* Words of the packed weight buffer of `shape`, or -1 (with the reason in
 * upkie_sim_last_error(NULL)) when the shape is out of range. */
int64_t upkie_mlp_packed_words(const UpkieMlpShape* shape);

/* One launch of the policy for num_envs envs: obs [num_envs][obs_dim], packed
 * [upkie_mlp_packed_words(shape)], calls [num_envs] (uint32, may be NULL when
 * deterministic), outputs norm_obs [num_envs][obs_dim], mean, action and
 * env_action [num_envs][act_dim], value and log_prob [num_envs]: contiguous
 * device buffers, every output may be NULL. With mean, action, env_action and
 * log_prob all NULL the actor does not run (and no counter advances); with
 * value NULL the critic does not run. No CPU fallback: UPKIE_ERR_NO_DEVICE
 * without a HIP device. Errors are reported through upkie_sim_last_error(NULL). */
int upkie_mlp_actor_critic(int32_t num_envs, const UpkieMlpShape* shape, const float* packed, const float* obs,
                           uint32_t* calls, uint64_t seed, int32_t deterministic, float* norm_obs, float* mean,
                           float* action, float* env_action, float* value, float* log_prob, void* stream);

/* Asymmetric actor-critic ("privileged observations"): with
 * shape->critic_obs_dim = Dc in 1-256 the critic reads a row of its own,
 *   xc    = clamp((critic_obs - critic_obs_mean) / critic_obs_std, -clip_obs, clip_obs)
 *           (xc = critic_obs when normalize == 0)
 *   value = critic(xc)
 * and everything of the actor is as above, on obs. The critic's first layer
 * takes Dc inputs; its statistics are one more fixed block of the packed
 * buffer, critic_obs_mean[Dcp], critic_obs_std[Dcp] (Dcp = Dc rounded up to
 * 4, std directly after mean: a pointer to the block serves as
 * upkie_vecnorm_step's packed_stats for a normaliser of Dc columns), after
 * action_high and before log_std, so the PPO update never writes it. With
 * critic_obs_dim == 0 every offset, upkie_mlp_packed_words and every output
 * are what they are without the field.
 * upkie_mlp_actor_critic_asym is upkie_mlp_actor_critic plus critic_obs
 * [num_envs][Dc] and the output norm_critic_obs [num_envs][Dc] (may be NULL;
 * written even when value is NULL); the same single launch: the critic's wave
 * reads its own pointer, width and statistics. It takes symmetric shapes too
 * (critic_obs is then [num_envs][obs_dim]). upkie_mlp_actor_critic refuses an
 * asymmetric shape (UPKIE_ERR_INVALID_ARGUMENT). */
int upkie_mlp_actor_critic_asym(int32_t num_envs, const UpkieMlpShape* shape, const float* packed, const float* obs,
                                const float* critic_obs, uint32_t* calls, uint64_t seed, int32_t deterministic,
                                float* norm_obs, float* norm_critic_obs, float* mean, float* action, float* env_action,
                                float* value, float* log_prob, void* stream);

/* ---- Privileged observation (the asymmetric critic's row) ---------------
 * One launch per env step that assembles, for every env n < num_envs, the row
 * the critic of an asymmetric actor-critic reads (csrc/privileged_obs.hpp).
 * The row is the concatenation of up to UPKIE_PRIVILEGED_MAX_SEGMENTS
 * segments, in the caller's order: segment k is kinds[k] with counts[k] words,
 *   UPKIE_PRIVILEGED_OBSERVATION: next_obs[n][0 .. count)   (the raw observation)
 *   UPKIE_PRIVILEGED_COMMAND:     command[n][0 .. count)    (what the env receives)
 *   UPKIE_PRIVILEGED_PUSH_FORCE:  force[c][n], c < count    ([count][num_envs]: the force the next step applies)
 *   UPKIE_PRIVILEGED_LINK_SCALE:  link_scale[links[c]][n]   ([*][num_envs]; links: count device int32 rows)
 * row_dim = the sum of the counts, 1-256. Pure data movement:
 *   new[n] = the row from the sources as they are at the call;
 *   final_observation[n] = new[n] where the episode goes on (done[n] ==
 *     terminated[n] | truncated[n] == 0); where it ended, the OBSERVATION
 *     words come from final_obs[n] (next_obs when final_obs is NULL) and every
 *     other word is the OLD observation[n] word: the command, force and scales
 *     that were current during the ended step (the sources already hold the
 *     next episode's). The old word is read before the new one is written, by
 *     the thread that writes it;
 *   observation[n] = new[n].
 * reset != 0: observation[n] = new[n] for the envs with mask[n] (done is the
 * mask; NULL: all), final_observation untouched. No allocation, no host
 * argument that changes between steps: capturable in a hipGraph. */
#define UPKIE_PRIVILEGED_MAX_SEGMENTS 8
enum UpkiePrivilegedKind {
  UPKIE_PRIVILEGED_OBSERVATION = 0,
  UPKIE_PRIVILEGED_COMMAND = 1,
  UPKIE_PRIVILEGED_PUSH_FORCE = 2,
  UPKIE_PRIVILEGED_LINK_SCALE = 3
};
int upkie_privileged_observation(int32_t num_envs, int32_t obs_dim, int32_t act_dim, int32_t num_segments,
                                 const int32_t* kinds, const int32_t* counts, const float* next_obs,
                                 const float* final_obs, const float* command, const float* force,
                                 const float* link_scale, const int32_t* links, const uint8_t* terminated,
                                 const uint8_t* truncated, int32_t reset, float* observation, float* final_observation,
                                 void* stream);

/* ---- Running observation / reward normalisation (VecNormalize) ----------
 * Stable-Baselines3's VecNormalize in training mode, on the device
 * (csrc/vecnorm.hpp): running statistics of the observations and of the
 * discounted returns, the reward scaled by the returns' running std. N =
 * num_envs, D = obs_dim (1-256). State, all fp64 device buffers:
 *   obs_stats [2 D + 1]: mean[D], var[D], count     (RunningMeanStd of obs)
 *   ret_stats [3]:       mean, var, count           (RunningMeanStd of returns)
 *   returns   [N]:       discounted return of every env
 * (RunningMeanStd(epsilon = 1e-4) starts at mean 0, var 1, count 1e-4.)
 * A batch x [N][D] updates (mean, var, count) with its fp64 mean bm and
 * population variance bv over the N rows:
 *   delta = bm - mean, tot = count + N
 *   mean += delta N / tot
 *   var   = (var count + bv N + delta^2 count N / tot) / tot,  count = tot
 * (bm and bv N come from per-lane Welford sums merged by Chan's formula in a
 * fixed order: the result is the same bits every call.)
 * One call, flags a set of UpkieVecNormFlag; done = terminated | truncated
 * (bytes, NULL: none); obs as the env returned it (with same-step autoreset,
 * the reset observation of the envs that ended):
 *   RESET:  returns[:] = 0; with TRAINING and NORM_OBS, obs updates obs_stats.
 *   else:   with TRAINING and NORM_OBS, obs updates obs_stats;
 *           with TRAINING, returns = returns gamma + reward and the N returns
 *           update ret_stats (whether or not NORM_REWARD is set);
 *           then returns[done] = 0.
 * Outputs (each may be NULL), computed with the statistics after the update:
 *   norm_reward[n]    = NORM_REWARD ? (float)clip(reward[n] / sqrt(ret_var + epsilon), +-clip_reward)
 *                       (in fp64, rounded once) : reward[n]
 *   norm_obs[n][d]    = NORM_OBS ? clip((obs[n][d] - mean_f32[d]) / std_f32[d], +-(float)clip_obs)
 *                       (in fp32: the MLP policy's expression, the same bits) : obs[n][d]
 *   episode_starts[n] = done[n] (uint8)
 * Whenever obs_stats move, the fp32 mirrors are rewritten: mean_f32[d] =
 * (float)mean[d], std_f32[d] = (float)sqrt(var[d] + epsilon), and, with a
 * policy's packed weight buffer in packed_stats (NULL: none), its obs_mean and
 * obs_std words: packed_stats[d] = mean_f32[d], packed_stats[Dp + d] =
 * std_f32[d], Dp = D rounded up to 4 (csrc/policy_mlp.hpp).
 * Launches: with TRAINING, one that reduces the moments (its last block
 * updates the statistics in place); a second one when a normalised reward or
 * normalised observations are asked for; without TRAINING, only the second.
 * No block waits on another, no float atomics, no allocation, no host
 * synchronisation: the call can be captured in a hipGraph and replayed.
 * workspace: upkie_vecnorm_workspace_bytes(N, D) bytes, zeroed once before
 * the first call (every call leaves its counter at zero again); needed with
 * TRAINING. No CPU fallback: UPKIE_ERR_NO_DEVICE without a HIP device. Errors
 * are reported through upkie_sim_last_error(NULL). */
enum UpkieVecNormFlag {
  UPKIE_VECNORM_TRAINING = 1,
  UPKIE_VECNORM_NORM_OBS = 2,
  UPKIE_VECNORM_NORM_REWARD = 4,
  UPKIE_VECNORM_RESET = 8
};

/* Bytes of the workspace for num_envs envs of obs_dim words, or -1 (with the
 * reason in upkie_sim_last_error(NULL)) out of range. Needs no device. */
int64_t upkie_vecnorm_workspace_bytes(int32_t num_envs, int32_t obs_dim);

int upkie_vecnorm_step(int32_t num_envs, int32_t obs_dim, const float* obs, const float* reward, const uint8_t* terminated,
                       const uint8_t* truncated, double* obs_stats, double* ret_stats, double* returns, void* workspace,
                       int32_t flags, double gamma, double epsilon, double clip_obs, double clip_reward, float* mean_f32,
                       float* std_f32, float* packed_stats, float* norm_obs, float* norm_reward, uint8_t* episode_starts,
                       void* stream);

/* Data-parallel form: W ranks (W >= 1), each with its own N_r envs, keep
 * one set of statistics, those of one normaliser over all sum_r N_r envs. A
 * step that moves a statistic (TRAINING, and NORM_OBS or not RESET) becomes
 *   upkie_vecnorm_moments_local(..., slot):  the returns update as in
 *     upkie_vecnorm_step; the batch moments of this rank's envs, per
 *     observation column d and for the returns (column D), go to slot:
 *       slot[c] = count, slot[D + 1 + c] = mean, slot[2 (D + 1) + c] = M2
 *     (c < D + 1; the columns the step does not reduce are not written); the
 *     statistics do not move. Launch A of upkie_vecnorm_step, and its per-env
 *     outputs when that step is one launch.
 *   the caller makes every rank's slot visible to every rank, unchanged:
 *     slots[r] = rank r's slot (slots[r] at slots + r * slot doubles);
 *   upkie_vecnorm_merge(..., slots, W): per column, (n, mean, M2) = slots[0],
 *     then Chan's merge of slots[1], ..., slots[W - 1] in rank order:
 *       delta = mean_r - mean, tot = n + n_r
 *       mean += delta n_r / tot,  M2 += M2_r + delta^2 n n_r / tot,  n = tot
 *     then the update above with bm = mean, bv N = M2 and N = n, the fp32
 *     mirrors and packed words as above, count += n; then the second launch
 *     of upkie_vecnorm_step when it has one.
 * Both take upkie_vecnorm_step's arguments, the same on both calls. Every
 * rank computes the same merge on the same bits: the statistics are the same
 * bits on every rank, and with W = 1 the same bits as upkie_vecnorm_step's.
 * slot: upkie_vecnorm_slot_bytes(D) bytes (8-byte aligned). */
int64_t upkie_vecnorm_slot_bytes(int32_t obs_dim);

int upkie_vecnorm_moments_local(int32_t num_envs, int32_t obs_dim, const float* obs, const float* reward,
                                const uint8_t* terminated, const uint8_t* truncated, double* obs_stats, double* ret_stats,
                                double* returns, void* workspace, int32_t flags, double gamma, double epsilon,
                                double clip_obs, double clip_reward, float* mean_f32, float* std_f32, float* packed_stats,
                                float* norm_obs, float* norm_reward, uint8_t* episode_starts, double* slot, void* stream);

int upkie_vecnorm_merge(int32_t num_envs, int32_t obs_dim, const float* obs, const float* reward, const uint8_t* terminated,
                        const uint8_t* truncated, double* obs_stats, double* ret_stats, double* returns, void* workspace,
                        int32_t flags, double gamma, double epsilon, double clip_obs, double clip_reward, float* mean_f32,
                        float* std_f32, float* packed_stats, float* norm_obs, float* norm_reward, uint8_t* episode_starts,
                        const double* slots, int32_t world, void* stream);

/* ---- PPO update of the MLP actor-critic --------------------------------
 * One minibatch of Stable-Baselines3's PPO.train for a MlpPolicy with separate
 * actor and critic towers (no gSDE), on the device (csrc/ppo.hpp), applied in
 * place to the packed weight buffer the rollout kernel reads. B = the
 * minibatch's samples, s = perm[minibatch_start + j], j < minibatch_size, of
 * the flattened [T N] rollout (obs [T N][obs_dim], actions [T N][act_dim]:
 * the raw Gaussian samples, old_values, old_log_prob, advantages, returns
 * [T N]); x = the observation normalised as upkie_mlp_actor_critic does
 * (unless config->obs_normalized: the buffer holds normalised observations).
 *   mu, value = the towers on x;  sigma_a = exp(log_std_a)
 *   log_prob  = sum_a -(act_a - mu_a)^2 / (2 sigma_a^2) - log_std_a - ln(2 pi) / 2
 *   adv       = (advantage - mean) / (std + 1e-8) over the minibatch (std
 *               unbiased; upkie_ppo_advantage_stats), or unchanged when
 *               normalize_advantage is off or B = 1
 *   ratio     = exp(log_prob - old_log_prob)
 *   policy_loss  = -mean(min(adv ratio, adv clamp(ratio, 1 - clip_range, 1 + clip_range)))
 *   values_pred  = clip_range_vf <= 0 ? value
 *                  : old_values + clamp(value - old_values, -clip_range_vf, clip_range_vf)
 *   value_loss   = mean((returns - values_pred)^2)
 *   entropy_loss = -sum_a (0.5 + ln(2 pi) / 2 + log_std_a)
 *   loss = policy_loss + ent_coef entropy_loss + vf_coef value_loss
 * g = d loss / d params, the gradient torch autograd gives for these
 * expressions (a tie of the minimum splits half / half, the clamps pass their
 * bounds); the parameters are every weight and bias of both towers (heads
 * included) and log_std -- the packed words from log_std's on; obs_mean /
 * obs_std and the action bounds are never written. Then clip_grad_norm_ and
 * torch.optim.Adam (m, v: [packed words] fp32 in the packed layout, zero
 * before the first step; adam_scalars[0] = lr, adam_scalars[1] = t, fp64):
 *   coef = min(1, max_grad_norm / (||g||_2 + 1e-6)),  g = coef g
 *   t += 1;  m = beta1 m + (1 - beta1) g;  v = beta2 v + (1 - beta2) g^2
 *   p -= (lr / (1 - beta1^t)) m / (sqrt(v) / sqrt(1 - beta2^t) + adam_eps)
 * Padding words of the packed layout have a zero gradient and stay zero.
 * stats[7] = policy_loss, value_loss, entropy_loss, loss, approx_kl =
 * mean((ratio - 1) - ln ratio), clip_fraction = mean(|ratio - 1| >
 * clip_range), ||g||_2 before the clip. Three launches (gradient partials per
 * block; their fold in a fixed order, whose last block forms ||g||, the clip
 * coefficient, the statistics and t; Adam), no float atomics: the result is
 * the same bits every call. No allocation, no host synchronisation, every
 * argument constant across training iterations: a sequence of calls can be
 * captured in a hipGraph and replayed. SB3's defaults: clip_range 0.2,
 * clip_range_vf None, ent_coef 0, vf_coef 0.5, max_grad_norm 0.5, Adam
 * betas (0.9, 0.999), eps 1e-5, lr 3e-4, normalize_advantage on. */
typedef struct {
  float clip_range;     /* > 0 */
  float clip_range_vf;  /* > 0, or <= 0 for None (no value clipping) */
  float ent_coef;
  float vf_coef;
  float max_grad_norm;  /* > 0 */
  float adam_beta1;     /* in [0, 1) */
  float adam_beta2;     /* in [0, 1) */
  float adam_eps;       /* > 0 */
  int32_t obs_normalized; /* 1: obs holds normalised observations (no transform) */
  int32_t reserved;       /* 0 */
} UpkiePpoConfig;

/* Bytes of the workspace of upkie_ppo_minibatch_update for `shape` (which
 * needs a critic) and minibatches of at most max_minibatch samples (<= 64 MiB
 * for every valid shape), or UPKIE_ERR_INVALID_ARGUMENT (the reason in
 * upkie_sim_last_error(NULL)). Needs no device. The workspace is zeroed once
 * before the first call; every call leaves its counter at zero again. */
int64_t upkie_ppo_workspace_bytes(const UpkieMlpShape* shape, int32_t max_minibatch);

/* For every minibatch j of an epoch (samples perm[j batch_size ..] of the
 * `total`, the last one short): adv_stats[j] = (mean, std + 1e-8) of its
 * advantages (fp64, std unbiased, a fixed order), or (0, 1) when normalize is
 * 0 or the minibatch has one sample. One launch. */
int upkie_ppo_advantage_stats(int32_t total, int32_t batch_size, const int32_t* perm, const float* advantages,
                              int32_t normalize, double* adv_stats, void* stream);

/* One minibatch (above): gradient, clip and Adam, and its stats row.
 * adv_stats: this minibatch's (mean, std + 1e-8) pair. Argument and shape
 * errors return UPKIE_ERR_INVALID_ARGUMENT before any device use; no CPU
 * fallback: UPKIE_ERR_NO_DEVICE without a HIP device. Errors are reported
 * through upkie_sim_last_error(NULL). */
int upkie_ppo_minibatch_update(const UpkieMlpShape* shape, const UpkiePpoConfig* config, int32_t total,
                               int32_t minibatch_start, int32_t minibatch_size, int32_t max_minibatch,
                               const int32_t* perm, const float* obs, const float* actions, const float* old_values,
                               const float* old_log_prob, const float* advantages, const float* returns,
                               const double* adv_stats, float* packed, float* adam_m, float* adam_v,
                               double* adam_scalars, void* workspace, float* stats, void* stream);

/* Data-parallel form: W ranks (W >= 1), each with its own rollout of the
 * same T N samples, the same minibatch size and a replica of the same
 * weights, train as one learner on the union: minibatch j of the union is
 * the union of the ranks' minibatches j, B_g = W B samples. Every exchange:
 * each rank writes its slot, the caller makes every rank's slot visible to
 * every rank unchanged (slots[r] = rank r's, contiguous), and every rank
 * folds them in rank order, so every rank computes the same bits.
 * Advantage statistics of an epoch (M minibatches; slot: 2 M doubles,
 * upkie_ppo_advantage_slot_bytes):
 *   upkie_ppo_advantage_partials(phase 0): slot[j] = sum of the minibatch's
 *     advantages (fp64, upkie_ppo_advantage_stats' order);
 *   exchange;
 *   upkie_ppo_advantage_partials(phase 1, slots, W): mean_j = sum_r
 *     slots[r][j] / (W B_j); slot[M + j] = sum of (advantage - mean_j)^2;
 *   exchange;
 *   upkie_ppo_advantage_finish(slots, W): adv_stats[j] = (mean_j,
 *     sqrt(sum_r slots[r][M + j] / (W B_j - 1)) + 1e-8), or (0, 1) when
 *     normalize is 0 or W B_j = 1.
 * A minibatch (slot: upkie_ppo_slot_bytes(shape)):
 *   upkie_ppo_minibatch_gradient(..., global_minibatch_size = W B, slot):
 *     the gradient of upkie_ppo_minibatch_update with the loss means over
 *     global_minibatch_size samples, summed over this rank's samples, without
 *     the entropy term: slot = g_r (fp32, packed words from log_std's on,
 *     padded to an even count), then the fp64 loss sums of the stats row
 *     (sum of min(surrogates), of (returns - values_pred)^2, of the
 *     approx_kl terms, the clipped count). The weights do not move;
 *   exchange;
 *   upkie_ppo_minibatch_apply(slots, W): g = g_0 + g_1 + ... + g_{W-1} in
 *     fp32 in rank order, minus ent_coef on the log_std words; then clip,
 *     Adam, t and the stats row (means over global_minibatch_size) exactly as
 *     upkie_ppo_minibatch_update.
 * With W = 1 (global_minibatch_size = minibatch_size) every output is the
 * same bits as upkie_ppo_advantage_stats' and upkie_ppo_minibatch_update's.
 * Same workspace as upkie_ppo_minibatch_update; slots 8-byte aligned. */
int64_t upkie_ppo_slot_bytes(const UpkieMlpShape* shape);

int64_t upkie_ppo_advantage_slot_bytes(int32_t total, int32_t batch_size);

int upkie_ppo_advantage_partials(int32_t total, int32_t batch_size, const int32_t* perm, const float* advantages,
                                 int32_t phase, const double* slots, int32_t world, double* slot, void* stream);

int upkie_ppo_advantage_finish(int32_t total, int32_t batch_size, int32_t normalize, const double* slots, int32_t world,
                               double* adv_stats, void* stream);

int upkie_ppo_minibatch_gradient(const UpkieMlpShape* shape, const UpkiePpoConfig* config, int32_t total,
                                 int32_t minibatch_start, int32_t minibatch_size, int32_t global_minibatch_size,
                                 int32_t max_minibatch, const int32_t* perm, const float* obs, const float* actions,
                                 const float* old_values, const float* old_log_prob, const float* advantages,
                                 const float* returns, const double* adv_stats, float* packed, void* workspace,
                                 void* slot, void* stream);

int upkie_ppo_minibatch_apply(const UpkieMlpShape* shape, const UpkiePpoConfig* config, int32_t global_minibatch_size,
                              int32_t max_minibatch, const void* slots, int32_t world, float* packed, float* adam_m,
                              float* adam_v, double* adam_scalars, void* workspace, float* stats, void* stream);

/* ---- PPO update, controlled form: schedules and target_kl ---------------
 * The hyper-parameters that change while training, and Stable-Baselines3's
 * target_kl early stop, live in a control block in device memory instead of
 * launch arguments, so that a captured update reads their current values and
 * can end early without a host synchronisation. control: UPKIE_PPO_CTRL_WORDS
 * doubles, 8-byte aligned, zeroed once by the caller; its first two words are
 * adam_scalars' (lr, t), so one block serves both forms. */
enum {
  UPKIE_PPO_CTRL_LR = 0,               /* Adam's learning rate */
  UPKIE_PPO_CTRL_T = 1,                /* Adam's step count: the minibatches applied */
  UPKIE_PPO_CTRL_CLIP_RANGE = 2,       /* > 0; read as a float, replaces config->clip_range */
  UPKIE_PPO_CTRL_CLIP_RANGE_VF = 3,    /* read as a float, replaces config->clip_range_vf; 0: none */
  UPKIE_PPO_CTRL_TARGET_KL = 4,        /* 0: no early stop */
  UPKIE_PPO_CTRL_STOPPED = 5,          /* 0 / 1: this update was stopped */
  UPKIE_PPO_CTRL_N_UPDATES = 6,        /* SB3's _n_updates: the epochs entered since the block was zeroed */
  UPKIE_PPO_CTRL_MINIBATCHES_RUN = 7,  /* statistics rows this update wrote, the stopping minibatch's included */
  UPKIE_PPO_CTRL_WORDS = 8
};

/* Writes lr, clip_range, clip_range_vf and target_kl (one launch on `stream`;
 * the other words are left alone). lr, clip_range_vf and target_kl finite and
 * >= 0, clip_range finite and > 0, or UPKIE_ERR_INVALID_ARGUMENT. Call it
 * between updates, not inside a captured sequence that should see new values:
 * a captured call replays the values it was captured with. */
int upkie_ppo_control_set(double* control, double lr, double clip_range, double clip_range_vf, double target_kl,
                          void* stream);

/* Starts an update: stopped = 0, minibatches_run = 0. One launch, capturable
 * in front of the update's minibatches. */
int upkie_ppo_update_begin(double* control, void* stream);

/* upkie_ppo_minibatch_update with the control block in place of adam_scalars.
 * Differences, in SB3's PPO.train order:
 *   - clip_range and clip_range_vf are the block's (config's are checked, not
 *     used);
 *   - if stopped is set on entry: stats[0..6] = NaN, nothing else is written;
 *   - otherwise n_updates += 1 when minibatch_start == 0 (an epoch is
 *     entered), minibatches_run += 1, the stats row is written, and if
 *     target_kl > 0 and approx_kl (the float32 of stats[4]) > 1.5 target_kl,
 *     stopped = 1: t, the weights, m and v are NOT updated by this minibatch
 *     nor by any later one until upkie_ppo_update_begin.
 * With target_kl = 0 and the block's clip values equal to config's, every
 * output is the same bits as upkie_ppo_minibatch_update's. Each of the three
 * launches reads one word more; a stopped minibatch still costs its three
 * launches, which return at once. */
int upkie_ppo_minibatch_update_controlled(const UpkieMlpShape* shape, const UpkiePpoConfig* config, int32_t total,
                                          int32_t minibatch_start, int32_t minibatch_size, int32_t max_minibatch,
                                          const int32_t* perm, const float* obs, const float* actions,
                                          const float* old_values, const float* old_log_prob, const float* advantages,
                                          const float* returns, const double* adv_stats, float* packed, float* adam_m,
                                          float* adam_v, double* control, void* workspace, float* stats, void* stream);

/* The data-parallel halves with a control block. The gradient half leaves the
 * slot as it is once stopped is set. The apply half takes the decision from
 * the exchanged slots' loss sums: every rank reads the same bits, so every
 * rank stops at the same minibatch (each rank holds its own block; they stay
 * equal). The caller cannot see the flag without a synchronisation, so it
 * goes on exchanging slots after a stop; those exchanges change nothing.
 * minibatch_start: this rank's, 0 for the first minibatch of an epoch. */
int upkie_ppo_minibatch_gradient_controlled(const UpkieMlpShape* shape, const UpkiePpoConfig* config, int32_t total,
                                            int32_t minibatch_start, int32_t minibatch_size,
                                            int32_t global_minibatch_size, int32_t max_minibatch, const int32_t* perm,
                                            const float* obs, const float* actions, const float* old_values,
                                            const float* old_log_prob, const float* advantages, const float* returns,
                                            const double* adv_stats, float* packed, void* workspace, void* slot,
                                            double* control, void* stream);

int upkie_ppo_minibatch_apply_controlled(const UpkieMlpShape* shape, const UpkiePpoConfig* config,
                                         int32_t minibatch_start, int32_t global_minibatch_size, int32_t max_minibatch,
                                         const void* slots, int32_t world, float* packed, float* adam_m, float* adam_v,
                                         double* control, void* workspace, float* stats, void* stream);

/* The gradient launch for an asymmetric shape (critic_obs_dim > 0; a
 * symmetric one is taken too): the existing signatures plus critic_obs
 * [total][Dc], the critic's rows of the same samples, and a nullable control
 * block (NULL: upkie_ppo_minibatch_update / _gradient, otherwise their
 * controlled forms). The actor's forward, loss and gradient read obs as
 * before; the critic's read critic_obs, normalised with critic_obs_mean /
 * critic_obs_std unless config->obs_normalized (which then holds for both
 * tensors). No term of the loss couples the towers before the norm clip, so
 * every gradient word is the symmetric arithmetic on its tower's own input.
 * upkie_ppo_workspace_bytes, the fold, apply, Adam and advantage-statistics
 * entry points serve both kinds of shape. The entry points without critic_obs
 * refuse an asymmetric shape. */
int upkie_ppo_minibatch_update_asym(const UpkieMlpShape* shape, const UpkiePpoConfig* config, int32_t total,
                                    int32_t minibatch_start, int32_t minibatch_size, int32_t max_minibatch,
                                    const int32_t* perm, const float* obs, const float* critic_obs, const float* actions,
                                    const float* old_values, const float* old_log_prob, const float* advantages,
                                    const float* returns, const double* adv_stats, float* packed, float* adam_m,
                                    float* adam_v, double* adam_scalars, double* control, void* workspace, float* stats,
                                    void* stream);

int upkie_ppo_minibatch_gradient_asym(const UpkieMlpShape* shape, const UpkiePpoConfig* config, int32_t total,
                                      int32_t minibatch_start, int32_t minibatch_size, int32_t global_minibatch_size,
                                      int32_t max_minibatch, const int32_t* perm, const float* obs,
                                      const float* critic_obs, const float* actions, const float* old_values,
                                      const float* old_log_prob, const float* advantages, const float* returns,
                                      const double* adv_stats, float* packed, void* workspace, void* slot,
                                      double* control, void* stream);

/* ---- PPO update with mirror symmetry: augmented samples, mirror loss ------
 * (rsl_rl's symmetry_cfg.) A mirror is a signed permutation per row kind:
 * (M_o x)[k] = obs_sign[k] x[obs_index[k]] for the observation, (act_index,
 * act_sign) for the action and, for an asymmetric shape, (critic_index,
 * critic_sign) for the critic's row. Each is an involution: index[index[k]]
 * == k and sign[index[k]] == sign[k]; a fixed point may carry either sign.
 * The mirrored partner of a stored sample s has
 *   - the stored rows M_o obs_s and M_c critic_obs_s; everything the update
 *     does to a stored row applies afterwards, unchanged: with obs_normalized
 *     = 0 the mirrored raw row is normalised with the statistics of word k;
 *     with obs_normalized = 1 the stored normalised row is mirrored as it is
 *     (under a live normaliser the mirror thus acts on normalised rows: a
 *     sign-flipped word with a non-zero running mean is slightly off);
 *   - the action M_a action_s (the raw Gaussian sample);
 *   - the original's old_log_prob, old_values, returns and normalised
 *     advantage (adv_stats are those of the B originals: the advantage
 *     statistics launch is unchanged).
 * P = the B originals plus, when augment, their B partners; n = |P|.
 *   loss = (1/n) sum over P [ -min(adv ratio, adv clamp(ratio))
 *                             + vf_coef (returns - values_pred)^2 ]
 *          + ent_coef entropy_loss + mirror_coef L_m
 *   L_m  = 1/(B A) sum_s sum_a ( mu(M_o x_s)[a]
 *                                - act_sign[a] sg(mu(x_s))[act_index[a]] )^2
 * sg stops the gradient: L_m trains through the mirrored forward only. L_m is
 * always computed and reported, also with mirror_coef = 0. Clip, tie and clamp
 * rules, the norm clip and Adam are upkie_ppo_minibatch_update's.
 * stats[UPKIE_PPO_MIRROR_STATS] = policy_loss and value_loss (means over n),
 * entropy_loss, loss (the mirror term included), approx_kl and clip_fraction
 * over the B ORIGINALS ONLY (a partner's ratio against the original's old
 * log-prob is not 1 before the first step unless the policy is symmetric, and
 * target_kl keeps its meaning), ||g||_2 before the clip, mirror_loss = L_m.
 * Three launches: the gradient launch runs 2 B positions (an original and its
 * partner adjacent in one 16-sample tile) whatever augment is; no float
 * atomics, the same bits every call. */
enum { UPKIE_PPO_MIRROR_STATS = 8 };

typedef struct {
  int32_t augment;    /* 0 / 1: the partners' surrogate and value terms count */
  float mirror_coef;  /* finite, >= 0 */
  const void* tables; /* DEVICE memory written by upkie_ppo_mirror_set */
} UpkiePpoMirror;

/* 32-bit words of the device table block of `shape` (index then sign of the
 * observation, of the critic's row, of the action), or
 * UPKIE_ERR_INVALID_ARGUMENT. Needs no device. */
int64_t upkie_ppo_mirror_words(const UpkieMlpShape* shape);

/* Validates the HOST tables (obs: [obs_dim], critic: [critic_obs_dim], act:
 * [act_dim]; index int32, sign float) and copies them to `tables` (device,
 * upkie_ppo_mirror_words words). Checked on the host before any device use:
 * every index in range, every sign +1 or -1, index an involution, partners'
 * signs equal; critic tables are required for an asymmetric shape and refused
 * (must be NULL) for a symmetric one. No unvalidated index ever reaches a
 * gather: the update reads `tables` only. Synchronises `stream`: call it once,
 * outside a capture. */
int upkie_ppo_mirror_set(const UpkieMlpShape* shape, const int32_t* obs_index, const float* obs_sign,
                         const int32_t* critic_index, const float* critic_sign, const int32_t* act_index,
                         const float* act_sign, void* tables, void* stream);

/* Bytes of the workspace of upkie_ppo_minibatch_update_mirror (the plain
 * layout for twice the positions and one loss sum more per block; zeroed once
 * before the first call). max_minibatch <= 2^30 - 1. Needs no device. */
int64_t upkie_ppo_mirror_workspace_bytes(const UpkieMlpShape* shape, int32_t max_minibatch);

/* One minibatch of the mirrored update (above). The arguments of
 * upkie_ppo_minibatch_update_asym -- critic_obs NULL for a symmetric shape,
 * control NULL for the plain form -- plus `mirror` and an 8-word stats row.
 * Capturable, no allocation, every argument constant across iterations. With
 * a control block it honours `stopped` as the controlled form does (all 8
 * words NaN, nothing else written) and stops on the ORIGINALS' approx_kl. */
int upkie_ppo_minibatch_update_mirror(const UpkieMlpShape* shape, const UpkiePpoConfig* config,
                                      const UpkiePpoMirror* mirror, int32_t total, int32_t minibatch_start,
                                      int32_t minibatch_size, int32_t max_minibatch, const int32_t* perm,
                                      const float* obs, const float* critic_obs, const float* actions,
                                      const float* old_values, const float* old_log_prob, const float* advantages,
                                      const float* returns, const double* adv_stats, float* packed, float* adam_m,
                                      float* adam_v, double* adam_scalars, double* control, void* workspace,
                                      float* stats, void* stream);

/* SB3's train/explained_variance of the critic over the `total` samples of a
 * rollout: out[0] = 1 - Var(returns - values) / Var(returns), population
 * variances, NaN when Var(returns) == 0. fp64, two passes (means, then
 * squared deviations) in a fixed order: the same bits every call. One launch
 * of one block.
 *   phase -1: one rank, everything in one launch (slots, slot unused).
 * Data-parallel form (W ranks of `total` samples each, slot: 4 doubles,
 * slots[r] = rank r's after an exchange; the sums in rank order):
 *   phase 0: slot[0..1] = sum of returns, sum of (returns - values);
 *   phase 1: slot[2..3] = the squared deviations about the global means;
 *   phase 2: out[0] from the slots (returns, values unused). */
int upkie_ppo_explained_variance(int32_t total, const float* returns, const float* values, int32_t phase,
                                 const double* slots, int32_t world, double* slot, double* out, void* stream);

/* ---- Policy distillation ------------------------------------------------
 * One minibatch of a supervised (behaviour-cloning) update of the ACTOR
 * tower of the MLP actor-critic of `shape`, on the device (csrc/distill.hpp),
 * in place on the packed weight buffer. B = the minibatch's samples, s =
 * perm[minibatch_start + j], j < minibatch_size, of `total` rows (obs
 * [total][obs_dim], labels [total][act_dim]: what a teacher would have done
 * on the sample); x = the observation normalised as upkie_mlp_actor_critic
 * does, unless obs_normalized; A = act_dim.
 *   mu   = the actor tower on x (the Gaussian's mean, NOT clamped to the
 *          action bounds)
 *   loss = 1 / (B A) sum_j sum_a (mu_a(x_j) - label_ja)^2
 * which is torch.nn.functional.mse_loss(mu, label). g = d loss / d params,
 * the gradient torch autograd gives: the head's dZ = 2 (mu - label) / (B A),
 * then the layers of the actor as in the PPO update (its forward, backward
 * and weight-gradient device functions, unchanged). The parameters are the
 * ACTOR's weights and biases (head included) alone: the partial gradients,
 * their fold, the norm and Adam range over exactly the actor's packed words,
 * every one of which every block writes (the layout's padding words too, as
 * zeros: the partials need no zeroed workspace; the zeroing is for the
 * fold's counter), so log_std, every critic word and
 * the fixed words before log_std (observation statistics, action bounds) are
 * neither read-modified nor written, and their words of adam_m and adam_v
 * stay what they were (0 under a fresh optimiser state). Then
 * clip_grad_norm_ and torch.optim.Adam as in the PPO update:
 *   coef = min(1, max_grad_norm / (||g||_2 + 1e-6)),  g = coef g
 *   t += 1;  m = beta1 m + (1 - beta1) g;  v = beta2 v + (1 - beta2) g^2
 *   p -= (lr / (1 - beta1^t)) m / (sqrt(v) / sqrt(1 - beta2^t) + adam_eps)
 * with lr = adam_scalars[0] and t = adam_scalars[1], fp64 words in DEVICE
 * memory (the first two words of a PPO control block serve): a captured
 * update follows a learning-rate schedule without a re-capture.
 * stats[UPKIE_DISTILL_STATS] = loss, ||g||_2 before the clip, coef. Three
 * launches (gradient partials per block; their fold in block order, whose
 * last block forms ||g||, coef, the statistics and t in a fixed order; Adam),
 * no float atomics: the same bits every call; no allocation, no host
 * synchronisation, every argument constant across iterations. Every shape
 * the PPO update takes is taken, asymmetric ones included (critic_obs_dim > 0
 * changes nothing here: the critic's rows are not read); a shape without a
 * critic is refused as there. The workspace (upkie_distill_workspace_bytes,
 * <= 64 MiB) is zeroed once before the first call. Argument and shape errors
 * return UPKIE_ERR_INVALID_ARGUMENT before any device use, the reason in
 * upkie_sim_last_error(NULL); no CPU fallback. */
enum { UPKIE_DISTILL_STATS = 3 };

int64_t upkie_distill_workspace_bytes(const UpkieMlpShape* shape, int32_t max_minibatch);

int upkie_distill_minibatch_update(const UpkieMlpShape* shape, int32_t total, int32_t minibatch_start,
                                   int32_t minibatch_size, int32_t max_minibatch, const int32_t* perm, const float* obs,
                                   const float* labels, float* packed, float* adam_m, float* adam_v, double* adam_scalars,
                                   double max_grad_norm, double adam_beta1, double adam_beta2, double adam_eps,
                                   int32_t obs_normalized, void* workspace, float* stats, void* stream);

/* The DAgger mix of a distillation rollout step, one launch, on the sim
 * handle (its seed and global env ids). Per env n < num_envs:
 *   r = Philox4x32-10(counter (global env id lo, hi, calls[n], 8 << 24), key
 *       = the handle's seed);  calls[n] += 1        (stream tag 8: the mix's)
 *   teacher = (r[0] >> 8) < threshold[0]
 *   applied[n][a] = clamp(teacher ? label[n][a] : student_action[n][a],
 *                         low[a], high[a]),  a < act_dim (1-64)
 *   drove[n] = teacher (a byte, 0 / 1)
 * threshold: ONE uint32 word in device memory, llround(beta 2^24) for a
 * probability beta that the teacher drives (0: never, 2^24: always), so that
 * a beta schedule moves under a captured rollout. Selection and clamp only:
 * exact. Keyed by the global env id: N envs are the same bits however they
 * are sharded. label, student_action, applied: [num_envs][act_dim]; low,
 * high: [act_dim]; calls: [num_envs], zeroed by the caller at a reset. */
int upkie_sim_distill_mix(UpkieSim* sim, int32_t act_dim, const uint32_t* threshold, const float* label,
                          const float* student_action, const float* low, const float* high, uint32_t* calls,
                          float* applied, uint8_t* drove, void* stream);

/* ---- Time-limit bootstrap (SB3 collect_rollouts) ----------------------
 * For every env n < num_envs with truncated[n] && !terminated[n] (bytes;
 * terminated may be NULL: none terminated), in place:
 *   reward[n] = fl32(reward[n] + fl32(fl32(gamma) * V(final_obs[n])))
 * two roundings, no contraction: what Stable-Baselines3's float32
 * `rewards[idx] += gamma * terminal_value` computes for an env that ended
 * by its time limit. V is the critic of the MLP actor-critic of `shape` on
 * the packed buffer, on final_obs [num_envs][obs_dim] normalised as
 * upkie_mlp_actor_critic does (the same packed obs_mean / obs_std words,
 * live when a normaliser writes them): bit for bit the value that
 * upkie_mlp_actor_critic writes for the same observation. Every other
 * reward keeps its bits. One launch, one wave per tile of 16 envs; a tile
 * without such an env loads no weight. No allocation, no host argument that
 * changes between steps: the call can be captured in a hipGraph. Needs a
 * critic (critic_layers > 0) and gamma in [0, 1]. SB3's order within a
 * rollout step: the Monitor statistics on the raw reward, VecNormalize, then
 * this on the normalised reward with the statistics after that update; its
 * semantics assume same-step autoreset (final_obs: the observation the
 * ended episode stopped in). Only the critic runs: for an asymmetric shape
 * (critic_obs_dim = Dc > 0) final_obs is the critic's final row
 * [num_envs][Dc], normalised with critic_obs_mean / critic_obs_std. No CPU
 * fallback: UPKIE_ERR_NO_DEVICE without a
 * HIP device. Errors are reported through upkie_sim_last_error(NULL). */
int upkie_mlp_bootstrap_time_limits(int32_t num_envs, const UpkieMlpShape* shape, const float* packed, const float* final_obs,
                                    const uint8_t* terminated, const uint8_t* truncated, double gamma, float* reward,
                                    void* stream);

/* ---- Episode statistics (SB3 Monitor + ep_info_buffer) -----------------
 * N = num_envs envs, a ring of `window` finished episodes (1-65536; SB3's
 * stats_window_size, 100 by default), csrc/episodes.hpp. State, device
 * buffers, zero before the first step:
 *   ep_return [N] fp64, ep_length [N] int32: the running episode of each env
 *   ring_return [window] fp64, ring_length [window] int32
 *   counters [3] int64: episodes finished so far, ring head, ring fill
 *   means [2] fp64: mean return, mean length over the ring (0 while empty)
 * One step (one launch), done[n] = terminated[n] | truncated[n] (bytes, NULL:
 * none):
 *   ep_return[n] += (double)reward[n];  ep_length[n] += 1   (every env; the
 *     fp64 sum in step order: Python's sum(Monitor.rewards), bit for bit)
 *   the envs with done[n] finish their episode (return, length) and their
 *   accumulators go back to 0; the step's K finished episodes, in increasing
 *   n, are appended to the ring: with K > window only the last `window` of
 *   them (a deque of maxlen window);
 *   counters[0] += K;  head = (head + min(K, window)) mod window;
 *   fill = min(fill + min(K, window), window);
 *   means[0] = (r_0 + r_1 + ... + r_{fill-1}) / fill in fp64, summed
 *     sequentially from the oldest entry to the newest;
 *   means[1] = (l_0 + ... + l_{fill-1}) / fill (integer sum, one rounding).
 * Monitor's round(r, 6) is not applied and there is no "t" (wall-clock)
 * entry. The ring's oldest entry is at (head - fill) mod window.
 * workspace: upkie_episodes_workspace_bytes(N) bytes, zeroed once before the
 * first step (every step leaves its counter at zero again). No block waits
 * on another, no float atomics, no allocation, no host synchronisation: the
 * same bits every call, and the step can be captured in a hipGraph.
 * upkie_episodes_reset: the accumulators of the envs with mask[n] != 0 (all
 * when mask is NULL) back to 0, no episode recorded, the ring kept
 * (Monitor.reset). No CPU fallback: UPKIE_ERR_NO_DEVICE without a HIP device.
 * Errors are reported through upkie_sim_last_error(NULL). */
int64_t upkie_episodes_workspace_bytes(int32_t num_envs);

int upkie_episodes_step(int32_t num_envs, int32_t window, const float* reward, const uint8_t* terminated,
                        const uint8_t* truncated, double* ep_return, int32_t* ep_length, double* ring_return,
                        int32_t* ring_length, int64_t* counters, double* means, void* workspace, void* stream);

int upkie_episodes_reset(int32_t num_envs, const uint8_t* mask, double* ep_return, int32_t* ep_length, void* stream);

/* ---- Evaluation tally (SB3 evaluate_policy's bookkeeping) ---------------
 * N = num_envs envs give E = n_eval_episodes episodes between them, E at most
 * `capacity`, the length of the record buffers (csrc/eval_episodes.hpp).
 * State, device buffers:
 *   ep_return [N] fp64, ep_length [N] int32: the running episode of each env
 *   count [N] int32: episodes the env has given
 *   target [N] int32: its quota, target[n] = (E + n) / N (integer division;
 *     the quotas sum to E; with N > E only the last E envs count, as in SB3)
 *   rec_return [capacity] fp64, rec_length, rec_env [capacity] int32,
 *   rec_truncated [capacity] bytes: the records, E of them when full
 *   counters [2] int64: filled (records so far), steps (steps begun with
 *     filled < E: what the evaluation took)
 *   summary [7] fp64, see below
 * upkie_eval_reset (one launch): ep_return, ep_length, count, counters and
 * summary to 0, target written for E. The records are not cleared: those
 * behind `filled` mean nothing.
 * One step (one launch), for every env n with count[n] < target[n] (an env at
 * its quota is left alone), term = terminated[n] != 0, trunc = truncated[n]
 * != 0 (bytes, NULL: none):
 *   ep_return[n] += (double)reward[n];  ep_length[n] += 1   (the fp64 sum in
 *     step order, as Python's sum over the episode's rewards)
 *   with term | trunc: the record (ep_return[n], ep_length[n], n,
 *     trunc & !term) is appended, count[n] += 1 and the accumulators go back
 *     to 0.
 *   The step's records are appended at `filled` in increasing n, so that the
 *   list is step-major and env-minor: the order SB3's loop appends in. The
 *   list cannot overflow (the quotas sum to E); every store is bounded by E
 *   all the same.
 * In the step in which filled reaches E, and in no other, summary is written
 * from the records r_k, l_k, t_k, k = 0 .. E - 1, in that order:
 *   [0] mean_r = (r_0 + r_1 + ... + r_{E-1}) / E, fp64, summed sequentially
 *   [1] ((r_0 - mean_r)^2 + ... + (r_{E-1} - mean_r)^2) / E, a second pass,
 *       sequential, every difference, square and sum rounded (no fused
 *       multiply-add): the population variance (numpy's std squared)
 *   [2] mean_l = (l_0 + ... + l_{E-1}) / E (integer sum, one rounding)
 *   [3] the same second pass over (double)l_k - mean_l
 *   [4] min r_k, [5] max r_k (x < min and x > max from r_0)
 *   [6] (t_0 + ... + t_{E-1}) / E: the share of episodes the time limit ended
 * Square roots are the host's. numpy sums pairwise, so np.mean of the same
 * records may differ in the last bits.
 * workspace: upkie_eval_workspace_bytes(N) bytes, zeroed once before the
 * first step (every step leaves its counter at zero again). No block waits
 * on another, no float atomics, no allocation, no host synchronisation, no
 * host argument that changes between steps: the same bits every call, and the
 * step can be captured in a hipGraph. Bad sizes and NULL buffers are refused
 * before any device use. No CPU fallback: UPKIE_ERR_NO_DEVICE without a HIP
 * device. Errors are reported through upkie_sim_last_error(NULL). */
int64_t upkie_eval_workspace_bytes(int32_t num_envs);

int upkie_eval_reset(int32_t num_envs, int32_t capacity, int32_t n_eval_episodes, double* ep_return, int32_t* ep_length,
                     int32_t* count, int32_t* target, int64_t* counters, double* summary, void* stream);

int upkie_eval_step(int32_t num_envs, int32_t capacity, int32_t n_eval_episodes, const float* reward, const uint8_t* terminated,
                    const uint8_t* truncated, double* ep_return, int32_t* ep_length, int32_t* count, const int32_t* target,
                    double* rec_return, int32_t* rec_length, int32_t* rec_env, uint8_t* rec_truncated, int64_t* counters,
                    double* summary, void* workspace, void* stream);

/* ---- Agent pipeline (action shaping, noise, VecFrameStack) --------------
 * What an agent wraps around the env before PPO sees it, csrc/
 * agent_pipeline.hpp: N = num_envs envs, D = obs_dim words per env
 * observation, A = act_dim (1-64), K = stack frames (>= 1) of
 * F = D + (A with ACTION_IN_OBSERVATION) words, K F <= 256 (the obs_dim cap of
 * upkie_mlp_actor_critic, which reads the stack). State, device buffers, zero
 * before the first reset:
 *   prev_command [N][A] float32: the command last sent to the env
 *   observation [N][K][F] float32: the stack, oldest frame first
 *     (Stable-Baselines3's VecFrameStack on a flat observation)
 *   calls [N] uint32: the call counter of the env's noise
 * Settings, the arguments every launch begins with: flags, a set of
 * UpkiePipelineFlag; dt > 0; action_lag (s; read with ACTION_LAG only);
 * params, a DEVICE buffer of 3 A + D float32 words low[A], high[A], action
 * sigma[A], observation sigma[D]; seed. upkie_pipeline_params checks HOST
 * arrays (low <= high, sigmas non-negative and finite; a NULL sigma array: all
 * zero) and packs them into `params` (host, may be NULL: check only); it
 * returns the word count 3 A + D or a negative status. dt and alpha =
 * dt / action_lag are rounded to float32 once; the arithmetic below is
 * float32, fl() one rounding, fma() a fused multiply-add, clip(v) =
 * min(max(v, low[a]), high[a]).
 *
 * upkie_pipeline_shape_action (one launch, between the policy and the env):
 * action [N][A] is the policy's env_action. Per word, p = prev_command, each
 * stage only with its flag:
 *   INTEGRATE_ACTION: u = clip(fma(action, dt, p)), otherwise u = action
 *   ACTION_NOISE:     u = clip(fma(sigma_a[a], z, u))
 *   ACTION_LAG:       c = fma(alpha, fl(u - p), p), otherwise c = u
 *     (utils/filters.py's low_pass_filter; alpha >= 0.5 is refused)
 *   command = c; prev_command = c.
 * A word whose action or result is not finite: command = 0 (the neutral
 * command) and prev_command keeps its value (the step kernels' rule).
 *
 * upkie_pipeline_observe (one launch, behind the env step): the new frame of
 * env n is fma(sigma_o[d], z, next_obs[n][d]) for d < D (next_obs[n][d] as it
 * is without OBSERVATION_NOISE), then command[n][0..A) with
 * ACTION_IN_OBSERVATION. done = terminated | truncated (bytes, NULL: none).
 *   not done: the stack moves one frame towards its old end, in place, and
 *     the new frame takes the last slot.
 *   done (same-step autoreset: next_obs is the reset observation):
 *     final_observation[n] = the OLD stack moved one frame with, in the last
 *     slot, the frame of final_obs[n] (noised with draws of its own, followed
 *     by the command that was just applied); then the stack is zero but for
 *     its last slot, which takes the frame of next_obs with a zero command,
 *     and prev_command[n] = 0. final_obs NULL (no same-step autoreset): the
 *     restart alone. The final_observation rows of envs that did not end keep
 *     what they held (the time-limit bootstrap reads truncated rows only).
 * upkie_pipeline_reset: that restart from obs for the envs with mask[n] != 0
 * (bytes, NULL: every env); the others keep their state.
 *
 * Noise: z is a standard normal from Philox4x32-10 with counter (n, calls[n],
 * 0, 5 << 24 | block) and key (seed lo, seed hi), Box-Muller on the block's
 * four words as upkie_mlp_actor_critic (whose tag is 4; the step kernels use
 * 0-3): element i & 3 of block i >> 2 for action word / observation column i,
 * block 64 + (i >> 2) for column i of the terminal frame. A launch that
 * draws (shape_action with ACTION_NOISE; observe with OBSERVATION_NOISE, every
 * env; reset with OBSERVATION_NOISE, the masked envs) reads calls[n] and
 * leaves calls[n] + 1: the draws of an env do not depend on the batch and a
 * saved counter resumes them. Without a noise flag no Philox round runs and
 * calls is not touched (it may be NULL).
 *
 * One wavefront serves whole envs; no allocation, no host synchronisation, no
 * host argument that changes between steps: every call can be captured in a
 * hipGraph. No CPU fallback: UPKIE_ERR_NO_DEVICE without a HIP device. Errors
 * are reported through upkie_sim_last_error(NULL). */
enum UpkiePipelineFlag {
  UPKIE_PIPELINE_ACTION_IN_OBSERVATION = 1,
  UPKIE_PIPELINE_INTEGRATE_ACTION = 2,
  UPKIE_PIPELINE_ACTION_NOISE = 4,
  UPKIE_PIPELINE_ACTION_LAG = 8,
  UPKIE_PIPELINE_OBSERVATION_NOISE = 16
};

int64_t upkie_pipeline_params(int32_t obs_dim, int32_t act_dim, const float* action_low, const float* action_high,
                              const float* action_noise, const float* observation_noise, float* params);

int upkie_pipeline_shape_action(int32_t num_envs, int32_t obs_dim, int32_t act_dim, int32_t stack, int32_t flags,
                                double dt, double action_lag, const float* params, uint64_t seed, const float* action,
                                float* prev_command, uint32_t* calls, float* command, void* stream);

int upkie_pipeline_observe(int32_t num_envs, int32_t obs_dim, int32_t act_dim, int32_t stack, int32_t flags, double dt,
                           double action_lag, const float* params, uint64_t seed, const float* next_obs,
                           const uint8_t* terminated, const uint8_t* truncated, const float* final_obs,
                           const float* command, float* prev_command, uint32_t* calls, float* observation,
                           float* final_observation, void* stream);

int upkie_pipeline_reset(int32_t num_envs, int32_t obs_dim, int32_t act_dim, int32_t stack, int32_t flags, double dt,
                         double action_lag, const float* params, uint64_t seed, const float* obs, const uint8_t* mask,
                         float* prev_command, uint32_t* calls, float* observation, void* stream);

/* ---- Reward terms (a declarative reward, per-term episode sums) ----------
 * The reference leaves the reward to the agent (upkie_env.py:230); this is
 * a reward of K weighted terms (1-16) over N = num_envs envs with raw
 * observations of D = obs_dim words (1-256) and actions of A = act_dim words
 * (1-64), evaluated in ONE launch per env step, csrc/reward_terms.hpp. State,
 * device buffers, zero before the first step, struct-of-arrays so that every
 * access of a wavefront is contiguous:
 *   prev_action [A][N] float32: the action of the env's previous step
 *   term_sum [K][N] fp64: per term the sum over the running episode
 *   term_last [K][N] fp64: the same of the env's last finished episode
 *   finished [N] int32: episodes the env has finished
 * Term k has n_k taps (1-8), a shape, a weight w_k and a scale s_k. A tap is
 * (source, index, fn, c): source one of UpkieRewardSource, index the word of
 * the source (below D for OBS, below A for ACTION and ACTION_RATE, ignored
 * otherwise), fn one of UpkieRewardFn, c its coefficient.
 * upkie_reward_terms_params checks HOST arrays (the per-term arrays hold K
 * entries, the tap arrays the taps of all terms one after another in term
 * order; sizes and indices in range, weights, coefficients and scales finite,
 * s_k > 0 for the shapes that read it, dt > 0 finite, clip_low <= clip_high
 * and neither NaN; infinite: no clamp) and packs the term table into `params`
 * (host, UPKIE_REWARD_PARAMS_BYTES bytes, may be NULL: check only), which the
 * caller copies to the device once; it returns that byte count or a negative
 * status. The table holds inv_dt = the float32 nearest 1 / dt (fp64 division):
 * the rate MULTIPLIES by it.
 *
 * upkie_reward_terms_step, per env e, float32 with one rounding fl() per
 * operation and no contraction unless fma() says so:
 *   ended = terminated[e] | truncated[e] (bytes; either may be NULL: 0)
 *   o = final_obs[e] if ended and final_obs is given, else next_obs[e]
 *     (same-step autoreset: next_obs of an ended env is the reset observation,
 *     final_obs the one its episode stopped in)
 *   a = action[e] ([N][A]: what the caller applied this step)
 *   source value: OBS o[index]; ACTION a[index]; ACTION_RATE
 *     fl(fl(a[index] - prev_action[index][e]) * inv_dt); ONE 1; TERMINATED
 *     1 if terminated[e] else 0 (a time limit does not set it)
 *   x_k = 0; over the taps in order: x_k = fma(c_j, g_j(source value), x_k),
 *     g the identity, sinf or cosf
 *   y_k by shape: IDENTITY x; ABS |x|; SQUARE fl(x x); EXP_ABS
 *     expf(-fl(|x| / s)); EXP_SQUARE q = fl(x / s), expf(-fl(q q)); DEADBAND
 *     t = fl(|x| - s), 0 if t < 0 else t
 *   v_k = fl(w_k y_k);  r = 0; over the terms in order: r = fl(r + v_k)
 *   reward[e] = clip_low if r < clip_low, clip_high if r > clip_high, else r
 *   term_sum[k][e] += (double)v_k   (fp64, in step order, unclamped)
 *   ended: term_last[k][e] = term_sum[k][e]; term_sum[k][e] = 0;
 *     finished[e] += 1; prev_action[.][e] = 0
 *   otherwise prev_action[.][e] = a.
 * Non-finite inputs pass through (comparisons with a NaN are false: it is
 * neither clamped nor dead-banded away): a poisoned term_sum lasts until the
 * env's episode ends.
 * upkie_reward_terms_reset: term_sum and prev_action of the envs with
 * mask[n] != 0 (all when mask is NULL) back to 0; term_last and finished are
 * kept, as upkie_episodes_reset keeps its ring.
 * obs_dim, act_dim and num_terms of a step must be the ones `params` was
 * packed for: a launch on another table writes nothing. No LDS, no atomics, no
 * block that reads what another writes, no allocation, no host
 * synchronisation, no host argument that changes between steps: the same bits
 * every call, and the step can be captured in a hipGraph. No CPU fallback:
 * UPKIE_ERR_NO_DEVICE without a HIP device. Errors are reported through
 * upkie_sim_last_error(NULL). */
#define UPKIE_REWARD_MAX_TERMS 16
#define UPKIE_REWARD_MAX_TAPS 8
#define UPKIE_REWARD_PARAMS_BYTES 2336

enum UpkieRewardSource {
  UPKIE_REWARD_OBS = 0,
  UPKIE_REWARD_ACTION = 1,
  UPKIE_REWARD_ACTION_RATE = 2,
  UPKIE_REWARD_ONE = 3,
  UPKIE_REWARD_TERMINATED = 4
};

enum UpkieRewardFn { UPKIE_REWARD_FN_ID = 0, UPKIE_REWARD_FN_SIN = 1, UPKIE_REWARD_FN_COS = 2 };

enum UpkieRewardShape {
  UPKIE_REWARD_IDENTITY = 0,
  UPKIE_REWARD_ABS = 1,
  UPKIE_REWARD_SQUARE = 2,
  UPKIE_REWARD_EXP_ABS = 3,
  UPKIE_REWARD_EXP_SQUARE = 4,
  UPKIE_REWARD_DEADBAND = 5
};

int64_t upkie_reward_terms_params(int32_t obs_dim, int32_t act_dim, int32_t num_terms, double dt, const int32_t* shapes,
                                  const float* weights, const float* scales, const int32_t* tap_counts,
                                  const int32_t* tap_sources, const int32_t* tap_indices, const int32_t* tap_fns,
                                  const float* tap_coefs, double clip_low, double clip_high, void* params);

int upkie_reward_terms_step(int32_t num_envs, int32_t obs_dim, int32_t act_dim, int32_t num_terms, const void* params,
                            const float* next_obs, const float* action, const uint8_t* terminated,
                            const uint8_t* truncated, const float* final_obs, float* prev_action, double* term_sum,
                            double* term_last, int32_t* finished, float* reward, void* stream);

int upkie_reward_terms_reset(int32_t num_envs, int32_t act_dim, int32_t num_terms, const uint8_t* mask,
                             float* prev_action, double* term_sum, void* stream);

/* ---- Rollout consumer (BASELINE.json configs[3]) ---
 * Generalized advantage estimation over a rollout resident in HBM: rewards,
 * values, episode_starts, advantages, returns are [num_steps][num_envs]
 * (episode_starts[t][n] != 0 when step t is the first of an episode),
 * last_values / last_dones [num_envs] describe the state after the last step.
 * The reference has no learner (README.md:107-109 points to external RL
 * playgrounds); the recurrence is the published one (Schulman et al. 2016).
 * Errors are reported through upkie_sim_last_error(NULL). */
int upkie_rollout_gae(int32_t num_steps, int32_t num_envs, const float* rewards, const float* values,
                      const uint8_t* episode_starts, const float* last_values, const uint8_t* last_dones,
                      double gamma, double gae_lambda, float* advantages, float* returns, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* UPKIE_HIP_H_ */
