/* jiminy_hip.h -- C ABI of the MI355X-native batched rigid-body dynamics library.
 *
 * This is the drop-in boundary for ONE hot path of duburcqa/jiminy: the per-step
 * physics (ABA forward dynamics with rotor armature + spring-damper contact
 * forces + SimpleMotor law + explicit Euler / RK4 step on the configuration
 * manifold + the RNEA-style "extra terms" + noiseless sensors), batched one robot
 * per wavefront lane on gfx950.
 *
 * What each entry point replaces in the reference (paths relative to the
 * reference tree, duburcqa/jiminy @ v1.8.12):
 *
 *   jm_model_create     Robot::pinocchioModel_ + motors/sensors/contact registries as seen
 *                       by the engine (core/src/robot/model.cc, robot.cc; built on the Python
 *                       side by jiminy_py/robot.py:518-860).  Binding replaced:
 *                       python/jiminy_pywrap/src/robot.cc (Robot.initialize, attach_motor, ...)
 *   jm_batch_create     Engine::add_robot + RobotState/StepperState allocation
 *                       (core/include/jiminy/core/engine/engine.h:134-156, 216-250;
 *                        python/jiminy_pywrap/src/engine.cc:600-606)
 *   jm_batch_bind       the numpy views on Eigen buffers (`DEF_READONLY` on RobotState::q...,
 *                       python/jiminy_pywrap/src/engine.cc:173-188): here the caller owns
 *                       the memory and lends device pointers
 *   jm_batch_set_options Engine::setOptions, hot-path subset (core/src/engine/engine.cc:2654-2795)
 *   jm_batch_start      Engine::start (core/src/engine/engine.cc:952-1533)
 *   jm_batch_stop       Engine::stop (core/src/engine/engine.cc:2419-2460)
 *   jm_batch_step       Engine::step fixed-step branch (core/src/engine/engine.cc:1724-2417)
 *                       = AbstractStepper::tryStep (core/src/stepper/abstract_stepper.cc:15-62)
 *                       + computeAllExtraTerms (engine.cc:800-915) + computeSensorMeasurements
 *   jm_batch_dynamics   Engine::computeRobotsDynamics (core/src/engine/engine.cc:3585-3708;
 *                       python binding `compute_robots_dynamics`, pywrap engine.cc:634-638)
 *   jm_batch_reset_lanes BaseJiminyEnv.reset state injection for a subset of the batch
 *                       (python/gym_jiminy/common/gym_jiminy/common/envs/generic.py:521-760)
 *   jm_last_error       JIMINY_THROW message text (core/include/jiminy/core/macros.h:82-86)
 *
 * Conventions: all batch arrays are structure-of-arrays `X[component][B]` (component-major,
 * lane-contiguous) of the batch scalar type (float64 or float32), living in device memory
 * owned by the caller.  Spatial vectors are [linear; angular], quaternions xyzw, free-flyer
 * velocity is expressed in the body frame (engine.cc:3591-3592).
 * All functions return 0 on success and a negative JM_E* code otherwise; they never throw.
 * Numerical failures are per lane: see the `status` field.
 */
#ifndef JIMINY_HIP_H
#define JIMINY_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- error codes (mapped by the Python facade to the exception classes of
 *      python/jiminy_pywrap/src/module.cc:96-103) */
#define JM_OK 0
#define JM_EINVAL (-1)      /* std::invalid_argument  -> ValueError   */
#define JM_ERUNTIME (-2)    /* std::runtime_error     -> RuntimeError */
#define JM_ECONTROLFLOW (-3)/* jiminy::bad_control_flow -> BadControlFlow */
#define JM_ELOOKUP (-4)     /* jiminy::lookup_error   -> LookupError  */
#define JM_ENOTIMPL (-5)    /* jiminy::not_implemented_error -> NotImplementedError */
#define JM_ETOPOLOGY (-6)   /* model topology does not match the compiled-in specialisation */

/* ---- joint type codes (core/include/jiminy/core/fwd.h:84-96 groups them as
 *      LINEAR / ROTARY / ROTARY_UNBOUNDED / FREE; the axis variant is explicit here) */
enum {
    JM_JT_NONE = 0,
    JM_JT_RX = 1, JM_JT_RY = 2, JM_JT_RZ = 3, JM_JT_RU = 4,
    JM_JT_PX = 5, JM_JT_PY = 6, JM_JT_PZ = 7, JM_JT_PU = 8,
    JM_JT_RUBX = 9, JM_JT_RUBY = 10, JM_JT_RUBZ = 11, JM_JT_RUBU = 12,
    JM_JT_FREEFLYER = 13,
    /* spherical joint (nq = 4: unit quaternion x y z w, nv = 3: angular velocity in the joint frame): the reference inserts
     * them as FLEXIBILITY joints (Model::addFlexibilityJointsToExtendedModel, core/src/robot/model.cc:1087-1165) and
     * applies a spring-damper on their rotation (Engine::computeInternalDynamics, core/src/engine/engine.cc:3365-3391).
     * One-robot-per-lane kernels. */
    JM_JT_SPHERICAL = 14
};

/* ---- scalar type of a batch */
enum { JM_F64 = 0, JM_F32 = 1 };

/* ---- ODE solvers (core/include/jiminy/core/engine/engine.h:30-38 `odeSolver`) */
enum { JM_SOLVER_EULER_EXPLICIT = 0, JM_SOLVER_RUNGE_KUTTA_4 = 1, JM_SOLVER_RUNGE_KUTTA_DOPRI = 2 };

/* ---- motor flags */
enum { JM_MOTOR_EFFORT_LIMIT = 1, JM_MOTOR_VELOCITY_LIMIT = 2, JM_MOTOR_FRICTION = 4 };

/* number of doubles per motor in `motor_params`:
 * reduction, effortLimit, velocityLimit, velocityEffortInvSlope,
 * frictionViscousPositive, frictionViscousNegative, frictionDryPositive,
 * frictionDryNegative, frictionDrySlope  (core/src/hardware/basic_motors.cc:83-143) */
#define JM_MOTOR_NPARAMS 9

/* ---- per-lane status bits written by the kernels (JM_F_STATUS).  The contract ("Lane status contract"):
 *  - the status of a lane belongs to that lane alone: a failed robot changes no number of another robot of the batch;
 *  - `start`, `step` and the masked lanes of `reset_lanes` OVERWRITE the status: every bit then describes that launch and
 *    nothing older.  NAN: the incoming q / v / a of a step or an acceleration of any evaluation of the launch; OUT_OF_BOUNDS
 *    (spring-damper model only): any evaluation of the launch, `lower <= q <= upper` is inside; FORCE_OVERFLOW: `start` and
 *    `reset_lanes` only, so the next step clears it; SOLVER_FAILURE: the LAST evaluation of the launch only;
 *  - the refresh launch that closes an adaptive interval (extra terms, sensors) ORs its bits into the status;
 *  - the adaptive stepper zeroes the status when `new_step` is set and carries it over otherwise; a lane that holds NAN or
 *    STEPPER_FAILURE is frozen (neither state nor stepper state moves, `t` stays behind `t_next`) until the next call with
 *    `new_step` or until `reset_lanes` -- the reference raises for its one robot there (engine.cc:2340-2384). */
enum {
    JM_LANE_OK = 0,
    JM_LANE_NAN = 1,            /* NaN in q/v/a (engine.cc:1737-1747, abstract_stepper.cc:41-48) */
    JM_LANE_OUT_OF_BOUNDS = 2,  /* a bounded joint left [lower, upper]: the reference would switch
                                   to its constraint solver (engine.cc:3285-3298, 3722) */
    JM_LANE_FORCE_OVERFLOW = 4, /* initial contact force > 1e5 N (engine.cc:1338-1345) */
    JM_LANE_STEPPER_FAILURE = 8,/* adaptive stepper: step size below 1e-10 s or too many successive
                                   failed iterations (engine.cc:2340-2384 raises for the robot) */
    JM_LANE_SOLVER_FAILURE = 16 /* constraint model: the PGS solver hit its iteration cap on the last
                                   evaluation (engine.cc:3755-3768 counts `successiveSolveFailed`) */
};

/* ---- model description: plain arrays, all host memory, copied by jm_model_create.
 * Joint 0 is the universe. Matrices are row-major 3x3. */
/* kinds of user constraint frames (jm_model_desc::cframe_kind) */
enum { JM_XKIND_FRAME = 0, JM_XKIND_SPHERE = 1, JM_XKIND_WHEEL = 2, JM_XKIND_DISTANCE = 3 };

typedef struct jm_model_desc {
    int32_t njoints, nq, nv;
    int32_t nmotors, ncontacts;
    int32_t nimu, nforce, ncontact_sensors, nencoder, neffort;
    const int32_t * parents;       /* [njoints] */
    const int32_t * jtypes;        /* [njoints] JM_JT_* */
    const int32_t * idx_q;         /* [njoints] */
    const int32_t * idx_v;         /* [njoints] */
    const double * axes;           /* [njoints*3] unit axis (unaligned joints) */
    const double * placement_R;    /* [njoints*9] joint placement wrt parent joint */
    const double * placement_p;    /* [njoints*3] */
    const double * mass;           /* [njoints] */
    const double * com;            /* [njoints*3] */
    const double * inertia;        /* [njoints*9] rotational inertia about the COM */
    const double * rotor_inertia;  /* [nv] armature on joint side */
    const double * position_lower; /* [nq] */
    const double * position_upper; /* [nq] */
    const int32_t * motor_joint;   /* [nmotors] */
    const int32_t * motor_flags;   /* [nmotors] JM_MOTOR_* */
    const double * motor_params;   /* [nmotors*JM_MOTOR_NPARAMS] */
    const int32_t * contact_joint; /* [ncontacts] parent joint of the contact frame */
    const double * contact_R;      /* [ncontacts*9] frame placement in the joint frame */
    const double * contact_p;      /* [ncontacts*3] */
    const int32_t * imu_joint;     /* [nimu] */
    const double * imu_R;          /* [nimu*9] */
    const double * imu_p;          /* [nimu*3] */
    const int32_t * force_joint;   /* [nforce] */
    const double * force_R;        /* [nforce*9] */
    const double * force_p;        /* [nforce*3] */
    const int32_t * contact_sensor_contact; /* [ncontact_sensors] index into contacts */
    const int32_t * encoder_joint;          /* [nencoder] */
    const int32_t * encoder_joint_side;     /* [nencoder] 1 = joint side */
    const double * encoder_reduction;       /* [nencoder] */
    const int32_t * effort_motor;           /* [neffort] motor index */
    /* ABI 7 -- frames a user-registered FrameConstraint may hold (`robot.add_constraint(name, FrameConstraint(frame,
     * maskDoFs))`, core/src/constraints/frame_constraint.cc:27-35, python/jiminy_pywrap/src/constraints.cc): part of the
     * TOPOLOGY like the contact points (the kernels are specialised on parent joint and mask).  Bit d of the mask = dof d
     * of (x, y, z, rot x, rot y, rot z), world aligned, is fixed.  One-robot-per-lane kernels. */
    int32_t n_constraint_frames;
    const int32_t * cframe_joint;  /* [n_constraint_frames] parent joint of the frame */
    const int32_t * cframe_mask;   /* [n_constraint_frames] 6-bit mask of the fixed dofs */
    const double * cframe_R;       /* [n_constraint_frames*9] frame placement in the joint frame */
    const double * cframe_p;       /* [n_constraint_frames*3] */
    /* kind of every constraint frame (JM_XKIND_*), second parent joint (DistanceConstraint, else 0) and 8 parameters:
     * SphereConstraint (sphere_constraint.cc) radius, normal[3]; WheelConstraint (wheel_constraint.cc) radius, normal[3],
     * axis[3] (wheel axis in the frame); DistanceConstraint (distance_constraint.cc) -, position[3] of the second frame
     * in ITS parent joint.  Masks: frame = the user's, sphere / wheel = 0b000111 (three rows at the contact point),
     * distance = 0b000001 (one row). */
    const int32_t * cframe_kind;   /* [n_constraint_frames] */
    const int32_t * cframe_joint2; /* [n_constraint_frames] */
    const double * cframe_params;  /* [n_constraint_frames*8] */
    /* ... and the 1-dof joints (revolute / prismatic) a user-registered JointConstraint may hold on a row of its own, next
     * to the joint's bound constraint like in the reference (`robot.add_constraint(name, JointConstraint(joint))`,
     * core/src/constraints/joint_constraint.cc, model.cc:884-905).  One-robot-per-lane kernels; the branch-parallel kernels
     * keep the flag-bit-2 form on the joint's bound row (jm_batch_set_joint_locks). */
    int32_t n_constraint_joints;
    const int32_t * cjoint_joint;  /* [n_constraint_joints] */
    /* ABI 8.  Flexibility of the spherical joints (`model_options["dynamics"]["flexibilityConfig"]`: stiffness, damping per
     * axis; the `inertia` entry is the joint's rotor inertia): u_internal -= Jlog3(q) (stiffness * log3(q)) + damping * w,
     * engine.cc:3377-3390.  [3 * njoints], rows of the other joints ignored; NULL when the model has no spherical joint. */
    const double * flex_stiffness;
    const double * flex_damping;
} jm_model_desc;

/* ---- hot-path subset of the engine options, same names/defaults as the reference
 * (core/include/jiminy/core/engine/engine.h:273-325) */
typedef struct jm_options {
    double gravity[6];                 /* world.gravity, default (0,0,-9.81,0,0,0) */
    double contact_stiffness;          /* contacts.stiffness          1e6  */
    double contact_damping;            /* contacts.damping            2e3  */
    double contact_friction;           /* contacts.friction           1.0  */
    double contact_transition_eps;     /* contacts.transitionEps      1e-3 */
    double contact_transition_velocity;/* contacts.transitionVelocity 1e-2 */
} jm_options;

/* ---- bindable batch fields (jm_batch_bind).  Shapes are [rows][B]. */
enum {
    JM_F_Q = 0,            /* [nq]      in/out  RobotState::q            */
    JM_F_V = 1,            /* [nv]      in/out  RobotState::v            */
    JM_F_A = 2,            /* [nv]      in/out  RobotState::a            */
    JM_F_COMMAND = 3,      /* [nmotors] in      RobotState::command      */
    JM_F_U_MOTOR = 4,      /* [nmotors] out     RobotState::uMotor       */
    JM_F_U = 5,            /* [nv]      out     RobotState::u            */
    JM_F_F_EXTERNAL = 6,   /* [njoints*6] out   RobotState::fExternal (joint frame)   optional */
    JM_F_CONTACT_FORCES = 7,/* [ncontacts*6] out Robot::contactForces_ (contact frame) optional */
    JM_F_IMU = 8,          /* [nimu*6]   out  gyro(3), accel(3)  (basic_sensors.cc:142-164) */
    JM_F_FORCE = 9,        /* [nforce*6] out  (basic_sensors.cc:368-387) */
    JM_F_CONTACT = 10,     /* [ncontact_sensors*3] out (basic_sensors.cc:267-277) */
    JM_F_ENCODER = 11,     /* [nencoder*2] out Q,V (basic_sensors.cc:509-539) */
    JM_F_EFFORT = 12,      /* [neffort]  out  (basic_sensors.cc:604-618) */
    JM_F_ENERGY = 13,      /* [2] out kinetic, potential (engine.cc:808-810)       optional */
    JM_F_JOINT_FORCES = 14,/* [njoints*6] out data.f joint internal wrenches (engine.cc:878-887) optional */
    JM_F_CENTROIDAL = 15,  /* [15] out com(3), hg(6), dhg(6) (engine.cc:889-904)    optional */
    JM_F_STATUS = 16,      /* [1] int32 per lane, JM_LANE_* bits */
    JM_F_WORKSPACE = 17,   /* scratch, jm_batch_workspace_rows() rows */
    JM_F_CON_FLAGS = 18,   /* [n_flag_rows] int32 in/out: per constraint, bit 0 = enabled, bit 1 = reversed
                              (AbstractConstraintBase::isEnabled_, JointConstraint::isReversed_); joint rows, bit 2
                              (set by the caller, kept by the library): a user-registered JointConstraint holds the
                              joint (Model::addConstraint, core/src/robot/model.cc:926-936) -- the row is bilateral,
                              always enabled, its reference configuration taken at jm_batch_start; branch-parallel
                              topologies */
    JM_F_CON_DATA = 19,    /* [n_data_rows] in/out: JointConstraint::configurationRef_ per bounded joint, then
                              the Lagrange multipliers `lambda_` of every constraint row (PGS warm start: bounds, 4 per
                              contact point, 6 per user constraint frame), then FrameConstraint::transformRef_ of every
                              user constraint frame (translation 3, rotation 9 row-major; taken at jm_batch_start, the
                              caller may overwrite it: `constraint.reference_transform`).  JM_F_CON_FLAGS carries one
                              more row per user constraint frame after the contacts (bit 0, set by the caller: the
                              lane's robot holds that FrameConstraint), then one per user constraint joint; the latter
                              add one multiplier row each behind the frames' and one reference-configuration row each
                              behind the frames' reference transforms */
    JM_F_FRICTION = 20,    /* [1] in, optional: contacts.friction of every lane (domain randomisation of the ground
                              friction, gym_jiminy envs/locomotion.py:257-262); both contact models, every topology
                              (spring-damper on the one-robot-per-lane kernels: ABI 9), unbound = the batch-wide
                              contacts.friction option */
    JM_F_MODEL_LANE = 21,  /* [13 * njoints] in, optional: body parameters of every lane, rows per joint
                              mass | com 3 | inertia xx xy xz yy yz zz | joint placement translation 3 -- the
                              output of Model::addBiasedToExtendedModel (core/src/robot/model.cc:1166-1236: mass,
                              centre of mass, inertia and relative body position biases), one model per
                              environment; float64, every topology (the one-robot-per-lane kernels: ABI 9);
                              unbound = the model's own */
    JM_F_APPLIED = 22,     /* [6 * K] in, optional: world-aligned (force, moment) applied at K <= 4 frames of any
                              joint (jm_batch_set_applied_frames), i.e. the current value of the impulse /
                              profile forces of core/src/engine/engine.cc:1838-2016.  These are HELD values: the
                              caller owns their time schedule and cuts the launches at their breakpoints.  Forces that
                              are a spline of time need no schedule: jm_batch_set_process_forces (ABI 11), which the
                              kernels evaluate inside every dynamics evaluation and add to these rows.  Every topology
                              (the one-robot-per-lane kernels: ABI 9) */
    JM_F_GROUND_OFFSET = 23, /* [2] in, optional: (x, y) added to the world position at which every lane samples the height map
                              of jm_batch_set_ground -- every environment its own patch of one large terrain, the batched
                              form of one `world.groundProfile` per environment instance (gym_jiminy: a new random
                              ground per episode); unbound = (0, 0) */
    JM_F_FLEXIBILITY = 24, /* [6 * nspherical] in, optional (ABI 9): stiffness 3, damping 3 of every spherical (flexibility) joint, in
                              joint order, per lane -- `flexibilityConfig` randomised per environment the way
                              WalkerJiminyEnv._setup does per episode (gym_jiminy envs/locomotion.py:288-296); read by
                              Engine::computeInternalDynamics' flexibility efforts (core/src/engine/engine.cc:3365-3391);
                              unbound = jm_model_desc::flex_stiffness / flex_damping */
    JM_F_LANE_TIME = 25,   /* [1] float64 in/out, needed with process forces (ABI 11): the time of every lane at the start of
                              its next integrator step.  Kept by the kernels while process forces are registered:
                              `start` sets it to 0, every integrator step of a step launch advances it by `dt` (sub-steps
                              of one launch included), `reset_lanes` sets it to 0 for the masked lanes -- engine time for the
                              lanes never re-initialised, episode time for the others.  Every lane stores its own value, so a
                              captured graph carries no time argument. */
    JM_F_COUNT = 26
};

/* ---- `contacts.model = "constraint"` (the reference's default contact model, engine.h:273) and the
 * joint position bounds it enforces: options of the boxed forward dynamics
 * (core/src/solver/constraint_solvers.cc:335-448, core/src/engine/engine.cc:3253-3338, 3710-3866).
 * Constraint rows of one robot, in the reference's registry order (robot/model.h:40-46):
 *   one row per bounded 1-dof joint (`JointConstraint`, model joint order; continuous joints never
 *   activate and own no row), then 4 rows per contact point (`FrameConstraint` with the translation
 *   and the rotation about the ground normal fixed: x, y, z, torsion; core/src/robot/model.cc:817-823).
 * Float64 batches only.  With the adaptive stepper the constraint state of the active lanes travels with
 * them (gathered / scattered around every attempt); call jm_batch_set_constraint_options before
 * jm_batch_adaptive_workspace_rows, whose result depends on the contact model. */
enum { JM_CONTACT_SPRING_DAMPER = 0, JM_CONTACT_CONSTRAINT = 1 };
typedef struct jm_constraint_options {
    int32_t contact_model;      /* contacts.model: JM_CONTACT_*                      */
    int32_t pgs_iter_max;       /* PGS_MAX_ITERATIONS = 100 (engine.cc:62)            */
    double torsion;             /* contacts.torsion            0.0                    */
    double stabilization_freq;  /* contacts.stabilizationFreq  20.0 (Baumgarte)       */
    double regularization;      /* constraints.regularization  1e-3                   */
    double tol_abs;             /* stepper.tolAbs 1e-5: PGS tolerances (engine.cc:1372-1373) */
    double tol_rel;             /* stepper.tolRel 1e-4                                */
    /* ABI 6: Baumgarte frequency of the user-registered constraints (jm_batch_set_joint_locks).  In the reference they keep
     * gains of their own -- zero until `setBaumgarteFreq` is called on them -- and Engine::start only overwrites those of the
     * internal constraints (abstract_constraint.cc:88-98, engine.cc:1276-1285).  < 0: the gains of `stabilization_freq`
     * (what ABI 5 did); >= 0: critically damped gains of this frequency, 0 = a pure acceleration constraint. */
    double user_stabilization_freq;
} jm_constraint_options;

typedef struct jm_model jm_model;
typedef struct jm_batch jm_batch;

/* Topology signature the library was specialised for (see DESIGN.md "model compilation"). */
const char * jm_topology_signature(void);
/* ABI version of this header. */
int32_t jm_abi_version(void);

int32_t jm_model_create(const jm_model_desc * desc, jm_model ** out);
int32_t jm_model_destroy(jm_model * model);

/* `device` is the HIP device ordinal the batch lives on. */
int32_t jm_batch_create(const jm_model * model, int64_t batch_size, int32_t dtype,
                        int32_t device, jm_batch ** out);
int32_t jm_batch_destroy(jm_batch * batch);
int32_t jm_batch_set_options(jm_batch * batch, const jm_options * options);
/* Number of [B]-rows of scratch the caller must provide through JM_F_WORKSPACE. */
int32_t jm_batch_workspace_rows(const jm_batch * batch);
/* Constraint contact model: options (not while a simulation is running) and the row counts of the
 * per-lane constraint state the caller lends through JM_F_CON_FLAGS (int32), JM_F_CON_DATA and
 * JM_F_WORKSPACE (batch dtype; the delassus matrix J M^-1 J^T of every lane and the PGS vectors).
 * With JM_CONTACT_CONSTRAINT, start / step / dynamics / reset_lanes run the constrained evaluation:
 * joint-bound and contact constraints are switched with the reference's hysteresis
 * (engine.cc:3285-3298, 3145-3193) and the multipliers solved by projected Gauss-Seidel
 * (constraint_solvers.cc:107-333) on every dynamics evaluation. */
int32_t jm_batch_set_constraint_options(jm_batch * batch, const jm_constraint_options * options);
int32_t jm_batch_constraint_rows(const jm_batch * batch, int32_t * n_flag_rows, int32_t * n_data_rows,
                                 int32_t * n_workspace_rows);
/* world.groundProfile (core/include/jiminy/core/engine/engine.h:292-302, used by
 * computeContactDynamicsAtFrame, core/src/engine/engine.cc:3138-3145) as a height map: `heights` is a device
 * array `[ny][nx]` in the batch dtype, sampled at (x0 + ix dx, y0 + iy dy) with bilinear patches (height and
 * unit normal), flat continuation outside the grid; NULL = flat ground at z = 0.  Both contact models (the rows of
 * a contact constraint live in the local frame of the surface, FrameConstraint::setNormal), branch-parallel topologies. */
int32_t jm_batch_set_ground(jm_batch * batch, const void * heights, int32_t nx, int32_t ny, double x0, double y0,
                            double dx, double dy);
/* User-registered JointConstraints (`Model::addConstraint(name, JointConstraint)`, core/src/robot/model.cc:926-936;
 * python/jiminy_pywrap/src/robot.cc:215 `add_constraint`): tell the batch that joint rows of JM_F_CON_FLAGS may carry
 * bit 2, so that its launches take kernels built with the unbounded rows (the plain kernels of robots with
 * register-resident solves ignore the bit).  Branch-parallel topologies, constraint contact model; 0 = none any more. */
int32_t jm_batch_set_joint_locks(jm_batch * batch, int32_t on);

/* Frames that carry the JM_F_APPLIED wrenches (`Engine::registerImpulseForce` / `registerProfileForce`,
 * core/src/engine/engine.cc:1838-1935, accept any frame of the model): `offsets` = K x 3 frame positions in the frame of
 * their parent joint, `joints` = the K parent joint indices (NULL = all on the root joint); K <= 4, K = 0 disables.
 * Every dynamics evaluation adds the wrench to `fext[parent joint]` in the joint frame, like
 * `Engine::computeExternalForces` (engine.cc:3481-3560) through `convertForceGlobalFrameToJoint`. */
int32_t jm_batch_set_applied_frames(jm_batch * batch, int32_t k, const double * offsets, const int32_t * joints);
/* Process forces (ABI 11): wrench components that are a function of time, evaluated by the kernels inside EVERY dynamics
 * evaluation at the time of that evaluation, the way Engine::computeExternalForces calls a profile force
 * (core/src/engine/engine.cc:3482-3494) -- a(t+) refresh at t, RK4 stages at t + dt/2, t + dt/2, t + dt, the end-of-step
 * evaluation of either solver at t + dt (abstract_runge_kutta_stepper.cc:33-73, euler_explicit_stepper.cc:5-21), stage i of an
 * attempt of size dt of the adaptive stepper at t + c_i dt, c = 1/5, 3/10, 4/5, 8/9, 1, 1 (runge_kutta_dopri_stepper.h:21-23;
 * jm_batch_step_adaptive), `start`, `reset_lanes` and `dynamics` at the lane's current time; t = JM_F_LANE_TIME.  Component `row % 6` (force x y z, moment x y z,
 * world aligned) of frame `row / 6` of jm_batch_set_applied_frames is its JM_F_APPLIED value (zero when that field is unbound)
 * plus `scale * p(t)`, p the periodic cubic Hermite spline of PeriodicGaussianProcess (core/src/utilities/random.cc:322-458)
 * through `n_knots` knots `knot_spacing` apart: `values`, `grads` = device arrays `[n_knots][B]` of float64, one realisation
 * per lane, read at every evaluation (the caller may refill them in place between launches).  K <= 4, K = 0 disables; refused
 * while a simulation is running and on float32 batches. */
typedef struct jm_process_force {
    int32_t row;            /* 6 * frame + component */
    int32_t n_knots;
    double knot_spacing;    /* period = n_knots * knot_spacing */
    double scale;
    const double * values;  /* [n_knots][B] */
    const double * grads;   /* [n_knots][B] time derivatives at the knots */
} jm_process_force;
int32_t jm_batch_set_process_forces(jm_batch * batch, int32_t k, const jm_process_force * forces);
/* Lend a device pointer for one field; NULL unbinds an optional output. */
int32_t jm_batch_bind(jm_batch * batch, int32_t field, void * device_ptr);

/* Engine::start: from bound (q, v, command) compute a, extra terms and sensors;
 * checks the initial contact forces. `stream` is a hipStream_t (NULL = default). */
int32_t jm_batch_start(jm_batch * batch, void * stream);
/* Engine::stop (core/src/engine/engine.cc:2419-2460): the model may be re-configured again. */
int32_t jm_batch_stop(jm_batch * batch);
/* Engine::step fixed-step branch: `n_substeps` integrator steps of `dt` with the command
 * held. `command_changed` != 0 re-evaluates a(t+) with the current command before the
 * first sub-step (engine.cc:2030-2042); `update_sensors` != 0 refreshes the sensor outputs
 * at the end (engine.cc:2386-2410). */
int32_t jm_batch_step(jm_batch * batch, int32_t solver, double dt, int32_t n_substeps,
                      int32_t command_changed, int32_t update_sensors, void * stream);
/* Engine::computeRobotsDynamics: a = f(q, v) with the bound command; q_in/v_in are device
 * arrays [nq][B] / [nv][B]; a_out [nv][B]. Does not modify the bound state. */
int32_t jm_batch_dynamics(jm_batch * batch, const void * q_in, const void * v_in,
                          void * a_out, void * stream);
/* Re-initialise the lanes whose mask byte is non-zero from (q_init, v_init) ([nq][B], [nv][B]):
 * copies the state, zeroes a, then performs the `start` computation for those lanes only. */
int32_t jm_batch_reset_lanes(jm_batch * batch, const uint8_t * lane_mask,
                             const void * q_init, const void * v_init, void * stream);

/* Per-launch kernel timing with HIP events recorded on the launch stream around every kernel
 * `jm_batch_step` launch of this batch (start / reset / dynamics launches are not timed; up to 2048 launches between two summaries).  `jm_batch_timing_summary`
 * blocks until the recorded launches completed, returns their count and summed duration (ms)
 * and restarts the recording. */
int32_t jm_batch_enable_timing(jm_batch * batch, int32_t enable);
int32_t jm_batch_timing_summary(jm_batch * batch, int32_t * n_launches, double * total_ms);

/* ---- adaptive stepping: `odeSolver = "runge_kutta_dopri"`, the reference's default
 * (core/include/jiminy/core/stepper/runge_kutta_dopri_stepper.h, core/src/stepper/runge_kutta_dopri_stepper.cc,
 *  step-size selection of core/src/engine/engine.cc:2021-2222).  Every lane carries its own step size.
 * The caller lends (jm_batch_bind_adaptive):
 *   workspace  [jm_batch_adaptive_workspace_rows()][B] scalars of the batch dtype (stage derivatives),
 *   state_f64  [5][B] float64: t, dt, dtLargest, dtLargestPrev, (scratch) -- initialise t = 0 and the
 *              three step sizes to 1e-6 (StepperState::reset, engine.h:219-236, engine.cc:1176),
 *   state_i32  [7][B] int32: iter, iterFailed, successiveIterTooLarge, successiveIterFailed, (2 scratch rows,
 *              then the list of the lanes still active in the current attempt) = 0.
 * jm_batch_step_adaptive advances every lane from its `t` to the breakpoint `t_next` (the caller splits
 * Engine::step at controller / sensor breakpoints exactly as for the fixed-step solvers), then refreshes
 * the extra terms and, if asked, the sensors.  `new_step` != 0 on the first interval of an Engine::step
 * call (resets the successive-failure counters, clears the status row).  Lanes whose step size falls
 * below 1e-10 s or that fail more than `successive_iter_failed_max` times in a row get
 * JM_LANE_STEPPER_FAILURE (the reference raises for its single robot, engine.cc:2340-2384).
 * Process forces (jm_batch_set_process_forces) are evaluated at the time of every stage, lane time + c_i dt_try, in both forms
 * of the stepper; an accepted step advances JM_F_LANE_TIME by its size as it advances `t`, a rejected one leaves it; the a(t+)
 * refresh (`command_changed`) and the closing refresh evaluate at lane time.  The row the per-stage form keeps the stage times
 * in belongs to the library (allocated by jm_batch_bind_adaptive).
 * The call synchronises the stream once per attempt (active-lane count); `attempts_out` (optional)
 * receives the number of attempts, `max_attempts` bounds it. */
typedef struct jm_adaptive_options
{
    double tol_rel;                     /* stepper.tolRel  (1e-4) */
    double tol_abs;                     /* stepper.tolAbs  (1e-5) */
    double dt_max;                      /* stepper.dtMax */
    double dt_restore_threshold_rel;    /* stepper.dtRestoreThresholdRel (0.2) */
    int32_t successive_iter_failed_max; /* stepper.successiveIterFailedMax (1000) */
    int32_t form;                       /* 0: one persistent launch per interval where the topology has that kernel
                                           (jm_qdopri.h), 1: always the per-stage launches over compacted lanes */
} jm_adaptive_options;
int32_t jm_batch_adaptive_workspace_rows(const jm_batch * batch);
int32_t jm_batch_bind_adaptive(jm_batch * batch, void * workspace, double * state_f64, int32_t * state_i32);
int32_t jm_batch_step_adaptive(jm_batch * batch, double t_next, const jm_adaptive_options * options,
                               int32_t new_step, int32_t command_changed, int32_t update_sensors,
                               int32_t max_attempts, int32_t * attempts_out, void * stream);

/* ---- gym_jiminy pipeline blocks, batched: one lane = one environment.
 * Topology independent; arrays are device pointers in the dtype of the call, `[rows][B]`.
 *
 * jm_block_pd_controller ≙ `pd_controller` + `integrate_zoh`
 *   (python/gym_jiminy/common/gym_jiminy/common/blocks/proportional_derivative_controller.py:23-163):
 *   advances the command state (position, velocity, acceleration targets, `[3][M][B]`, in place) by
 *   one controller period under its bounds and writes the clipped PD torques `[M][B]`.
 *   `encoder` is the raw JM_F_ENCODER field (`[n_enc][2][B]`), `encoder_index[m]` the encoder of
 *   motor m; `lower` / `upper` are `[3][M]`, `kp`, `kd`, `effort_limit` `[M]` host arrays.
 * jm_block_mahony_filter ≙ `mahony_filter` (blocks/mahony_filter.py:28-101): `imu` is the raw
 *   JM_F_IMU field (`[n_imu][6][B]`), `quat` `[4][n_imu][B]` (xyzw) and `bias` `[3][n_imu][B]`
 *   are updated in place, `omega` / `cf` `[3][n_imu][B]` receive the de-biased rates. */
#define JM_BLOCK_MAX_MOTORS 40
int32_t jm_block_pd_controller(int32_t dtype, int64_t batch_size, int32_t nmotors, const void * encoder,
                               const int32_t * encoder_index, void * command_state,
                               const double * lower, const double * upper, const double * kp,
                               const double * kd, const double * effort_limit, double control_dt,
                               void * out_torque, void * stream);
int32_t jm_block_mahony_filter(int32_t dtype, int64_t batch_size, int32_t n_imu, const void * imu,
                               void * quat, void * omega, void * cf, void * bias, double kp, double ki,
                               double dt, void * stream);
/* jm_block_pd_adapter ≙ `pd_adapter` (proportional_derivative_controller.py:166-260), the `PDAdapter` block: from
 *   the action `[M][B]` (target motor position, `order` 0, or velocity, `order` 1) to the target acceleration
 *   `out` `[M][B]` held over `step_dt` (or, `is_instantaneous`, the command state `[3][M][B]` moved at once and a
 *   zero acceleration); `lower` / `upper` `[3][M]`, `velocity_deadband` `[M]` or NULL (host arrays).
 * jm_block_motor_safety_limit ≙ `apply_safety_limits` (blocks/motor_safety_limit.py:20-77), the `MotorSafetyLimit`
 *   block: clips the command torques `[M][B]` so that they act against soft position bounds / the velocity limit;
 *   `encoder` is the raw JM_F_ENCODER field, `encoder_index[m]` the encoder of motor m, the gains and limits are
 *   host arrays `[M]`. */
int32_t jm_block_pd_adapter(int32_t dtype, int64_t batch_size, int32_t nmotors, const void * action, int32_t order,
                            void * command_state, const double * lower, const double * upper,
                            int32_t is_instantaneous, const double * velocity_deadband, double step_dt,
                            void * out_acceleration, void * stream);
int32_t jm_block_motor_safety_limit(int32_t dtype, int64_t batch_size, int32_t nmotors, const void * encoder,
                                    const int32_t * encoder_index, const void * command, const double * kp,
                                    const double * kd, const double * soft_position_lower,
                                    const double * soft_position_upper, const double * velocity_limit,
                                    const double * effort_limit, void * out_command, void * stream);

/* ---- Sensor white noise and bias (sensor part), batched.
 *
 * jm_block_sensor_noise ≙ `AbstractSensorBase::measureData` (core/src/hardware/abstract_sensor.cc:71-85)
 *   and, with `rot_bias_inv`, `ImuSensor::measureData` (core/src/hardware/basic_sensors.cc:166-187),
 *   applied in place to one raw measurement field (`data`, device, `[n_sensors][n_fields][B]`, e.g.
 *   JM_F_IMU) right after the step that refreshed it: white noise `normal(generator, 0, noiseStd)`
 *   first (float ziggurat over a PCG32 stream, core/src/utilities/random.cc:10-167), then the additive
 *   bias, then (IMU) the rotation bias applied to both 3-vectors. `rng_state` (device, uint64
 *   `[n_sensors][B]`) is the PCG32 state of every (sensor, lane), advanced exactly as the reference
 *   advances `AbstractSensorBase::generator_`. `noise_std`, `bias` are host arrays
 *   `[n_sensors][n_fields]` (NULL = option left empty), `rot_bias_inv` a host array `[n_sensors][9]`
 *   (row-major `exp3(-bias.head<3>())`, basic_sensors.cc:121-129) or NULL.
 * jm_sensor_rng_seed ≙ the generator seeding of `AbstractSensorTpl<T>::resetAll(seed)`
 *   (core/include/jiminy/core/hardware/abstract_sensor.hxx:213-226): for every lane,
 *   `std::seed_seq{group_seed[lane]}.generate` of `n_sensors` words, sensor s gets the PCG32 state
 *   `word_s | 3`. Host arrays in, host array `[n_sensors][B]` out (upload it as `rng_state`). */
#define JM_NOISE_MAX_ROWS 128
#define JM_NOISE_MAX_FIELDS 6
#define JM_NOISE_MAX_ROT 8
int32_t jm_block_sensor_noise(int32_t dtype, int64_t batch_size, int32_t n_sensors, int32_t n_fields,
                              void * data, uint64_t * rng_state, const double * noise_std,
                              const double * bias, const double * rot_bias_inv, void * stream);
int32_t jm_sensor_rng_seed(const uint32_t * group_seed, int64_t batch_size, int32_t n_sensors,
                           uint64_t * state_out);

/* ---- Model biases per environment (model part), batched, drawn on the device.
 *
 * jm_block_model_bias ≙ `Model::addBiasedToExtendedModel(g)` (core/src/robot/model.cc:1166-1236) for every
 *   lane: for the mechanical joints in index order (`first_joint`..njoints-1: the free-flyer root is not one of
 *   them, model.cc:337-341) and in the reference's field order -- centre of mass (3 normals), mass (1), inertia
 *   (3 for the rotation vector of the principal axes, 3 for the principal moments), joint placement translation
 *   (3), each group only when its standard deviation is > EPS -- the lane's engine generator `rng_state[lane]`
 *   (device, uint64 `[B]`: the PCG32 stream of `Engine::generator_`) is advanced exactly as the reference advances
 *   it, the float normals are `normal(g, mean, std)` of core/src/utilities/random.cc:52-167, and the biased body
 *   parameters are written to the rows of `model_lane` (device, `[13 * njoints][B]`, JM_F_MODEL_LANE layout).
 *   `nominal` (device, float64 `[njoints][25]`): mass | com 3 | inertia xx xy xz yy yz zz | placement translation 3
 *   | principal moments 3 (ascending) | principal axes 9 (row-major, columns = axes) of the unbiased model.
 *   `std4` (host): inertia, mass, centre of mass, relative position standard deviations.  `mask` (device, uint8
 *   `[B]`) or NULL: only the masked lanes draw (episode-wise re-randomisation of the lanes being reset).
 * jm_engine_rng_seed ≙ `generator_.seed(std::seed_seq(randomSeedSeq))` (core/src/engine/engine.cc:756-757,
 *   random.hxx:20-51) with one seed word per lane: PCG32 state `(w0 | w1 << 32) | 3` of the two words
 *   `std::seed_seq{seed[lane]}` generates.  Host arrays. */
int32_t jm_block_model_bias(int32_t dtype, int64_t batch_size, int32_t njoints, int32_t first_joint,
                            const double * nominal, const float * std4, uint64_t * rng_state,
                            const uint8_t * mask, void * model_lane, void * stream);
int32_t jm_engine_rng_seed(const uint32_t * seed, int64_t batch_size, uint64_t * state_out);

/* ---- Sensor delay and jitter, batched.
 * jm_block_sensor_delay ≙ `AbstractSensorTpl<T>::interpolateData`
 *   (core/include/jiminy/core/hardware/abstract_sensor.hxx:305-429), the first half of `measureDataAll`: call it
 *   after every sensor refresh, before jm_block_sensor_noise.  `data` (device, `[n_sensors][n_fields][B]`) is
 *   overwritten with the measurement delayed by `delay[s] + uniform(0, jitter[s])` read from the history ring
 *   `history` (device, `[slots][n_sensors * n_fields][B]`, raw measurements the caller stored after each
 *   refresh, the current one included): zero-order hold (`order` 0) or linear interpolation (1), the oldest
 *   sample while the ring does not reach back far enough.  `slot[i]` / `times[i]` (host, i < n_history <= 64,
 *   ascending times, the last one the current time) name the ring slot and the time of the i-th oldest sample.
 *   The uniform number is drawn from `rng_state` (the generators of jm_block_sensor_noise) on every call,
 *   whether or not a jitter is configured, as the reference does; `history` NULL only takes that draw. */
#define JM_DELAY_MAX_HISTORY 64
int32_t jm_block_sensor_delay(int32_t dtype, int64_t batch_size, int32_t n_sensors, int32_t n_fields, void * data,
                              const void * history, const int32_t * slot, const double * times, int32_t n_history,
                              uint64_t * rng_state, const double * delay, const double * jitter,
                              int32_t interpolation_order, void * stream);

/* ---- DeformationEstimator observer block (ABI 10), batched: one lane = one environment.
 * jm_block_deformation_estimator ≙ `DeformationEstimator.refresh_observation`
 *   (python/gym_jiminy/common/gym_jiminy/common/blocks/deformation_estimator.py:831-863): from the encoders and the IMU
 *   attitude estimates (`imu_quat`, `[4][n_imu][B]` xyzw, e.g. the state of jm_block_mahony_filter) to one deformation
 *   quaternion per flexibility point (`out_quat`, `[4][n_flex][B]`) and, `out_rpy` not NULL, its roll-pitch-yaw angles
 *   (`[3][n_flex][B]`, `quat_to_rpy`, utils/math.py:158-201).  Per chain of interleaved IMU / flexibility frames
 *   `flexibility_estimator` (:139-235) = `_compute_orientation_error` (:30-76; `ignore_twist`: `compute_tilt_from_quat`
 *   + `swing_from_vector`, utils/math.py:1045-1133, else `matrices_to_quat` :306-360 + `quat_multiply` :570-626) then
 *   `_compute_deformation_from_deviation` (:80-134).  The rotations of the theoretical (rigid) model (:833-841) are
 *   evaluated on the device from the description below.
 * jm_deform_desc: the plan (host arrays, copied by jm_deform_plan_create).
 *   Frames: frame f is the product of its segments `frame_seg_start[f] .. frame_seg_start[f + 1] - 1`; a segment is a
 *   constant rotation `seg_rot` (row-major 3x3) followed by a joint rotation: `seg_kind` 0 none, 1 / 2 / 3 about x / y / z,
 *   4 about the unit vector `seg_axis`, by the angle `seg_ratio * encoder[seg_enc]` (position row of that encoder in the
 *   raw JM_F_ENCODER field `[n_enc][2][B]`; `seg_ratio` brings a motor-side encoder to the joint side).
 *   Chains: chain c has `chain_nflex[c]` flexibility points and `chain_nflex[c] + 1 - chain_orphan[c][1]` IMUs, listed
 *   in chain order in `chain_imu` (column of `imu_quat`) / `chain_imu_frame` (kinematic frame of that IMU) and in
 *   `flex_frame` (kinematic parent frame of the flexibility point, :776-788) / `flex_flipped` (:132-134); output column
 *   k is the k-th flexibility point of that concatenated order.  `chain_orphan[c]` ≙ `is_chain_orphan` (:641-647): [1] the
 *   last flexibility point of the chain has no IMU behind it; [0] (the FIRST IMU is missing) must be 0: the reference's
 *   block cannot be built for such a chain either (:297-307, :606-611).
 * jm_deform_plan_create validates the description (JM_EINVAL + jm_last_error, before any device call) and uploads it;
 * jm_block_deformation_estimator then allocates, copies and synchronises nothing: it can be captured into a HIP graph. */
typedef struct jm_deform_desc
{
    int32_t n_imu;          /* columns of imu_quat */
    int32_t n_enc;          /* sensors of the encoder field */
    int32_t n_flex;         /* columns of the outputs = sum of chain_nflex */
    int32_t ignore_twist;
    int32_t n_chain;
    const int32_t * chain_nflex;        /* [n_chain] */
    const int32_t * chain_orphan;       /* [n_chain][2] */
    const int32_t * chain_imu;          /* [sum of IMUs per chain] */
    const int32_t * chain_imu_frame;    /* same */
    const int32_t * flex_frame;         /* [n_flex] */
    const int32_t * flex_flipped;       /* [n_flex] */
    int32_t n_frame;
    const int32_t * frame_seg_start;    /* [n_frame + 1], ascending, last = n_seg */
    int32_t n_seg;
    const int32_t * seg_kind;           /* [n_seg] */
    const int32_t * seg_enc;            /* [n_seg], -1 where seg_kind is 0 */
    const double * seg_rot;             /* [n_seg][9] */
    const double * seg_axis;            /* [n_seg][3] */
    const double * seg_ratio;           /* [n_seg] */
} jm_deform_desc;
typedef struct jm_deform_plan jm_deform_plan;
int32_t jm_deform_plan_create(const jm_deform_desc * desc, jm_deform_plan ** out);
int32_t jm_deform_plan_destroy(jm_deform_plan * plan);
int32_t jm_block_deformation_estimator(const jm_deform_plan * plan, int32_t dtype, int64_t batch_size,
                                       const void * encoder, const void * imu_quat, void * out_quat, void * out_rpy,
                                       void * stream);

/* ---- Attitude observers: the `MahonyFilter` block around its filter function, and the `BodyObserver` block; batched, one
 * lane = one environment.  New symbols only: no existing structure or signature changed with them.
 * jm_attitude_desc: the plan (host arrays, copied by jm_attitude_plan_create).  Per IMU sensor (sensor order): the filter
 *   gains `kp`, `ki`, the rotation of the sensor frame relative to its parent body as a quaternion `rel_quat` (xyzw,
 *   `matrices_to_quat` rule) and the world rotation of the sensor frame as a list of segments
 *   `frame_seg_start[s] .. frame_seg_start[s + 1] - 1`: a segment is a constant rotation `seg_rot` (row-major 3x3) followed by a
 *   joint rotation read from the configuration rows `q` `[nq][B]` at `seg_q_index`: `seg_kind` 0 none, 1 / 2 / 3 about x / y / z
 *   by the angle `q[i]`, 4 about the unit vector `seg_axis` by `q[i]`, 5 about `seg_axis` with `(cos, sin) = q[i], q[i + 1]`
 *   (unbounded revolute joint), 6 the unit quaternion `q[i .. i + 3]` (xyzw: spherical joint, free-flyer orientation).
 *   Prismatic joints contribute nothing.  jm_attitude_plan_create validates the description (JM_EINVAL + jm_last_error,
 *   before any device call) and uploads it; the three calls then allocate, copy and synchronise nothing.
 * jm_block_attitude_init ≙ `MahonyFilter.refresh_observation` while the filter is not initialised
 *   (python/gym_jiminy/common/gym_jiminy/common/blocks/mahony_filter.py:340-374), on the lanes of `lane_mask` (device, uint8
 *   `[B]`; NULL: every lane; other lanes are not touched): `exact_init` the true orientation of the sensor frames from `q`,
 *   else `swing_from_vector` of the normalised accelerometer rows of `imu` (raw JM_F_IMU field `[n_imu][6][B]`), falling back
 *   to the true orientation on lanes where every accelerometer component is below 0.1 g.  Writes `quat` `[4][n_imu][B]`
 *   (xyzw), zeroes `omega`, `cf`, `bias` `[3][n_imu][B]` and `twist` `[n_imu][B]` (or NULL), writes `rpy` `[3][n_imu][B]` (or NULL).
 * jm_block_mahony_observer ≙ one later refresh (:376-393): `mahony_filter` with the gains of every IMU, then
 *   `remove_twist_from_quat` (`ignore_twist`) and `quat_to_rpy` (`rpy` not NULL) -- also after the filter's early return.
 * jm_block_body_observer ≙ `BodyObserver.refresh_observation` (blocks/body_orientation_observer.py:237-266):
 *   `quat = imu_quat * conj(rel_quat)`, `omega = rel_quat applied to imu_omega`, then by `twist_mode` 0 nothing, 1
 *   `remove_twist_from_quat`, 2 that and `update_twist` (:26-71) with the leak `max(0, 1 - time_constant_inv * dt)` on the
 *   state `twist` `[n_imu][B]` (NULL allowed for modes 0, 1); `rpy` or NULL.  `quat` must not alias `imu_quat`. */
typedef struct jm_attitude_desc
{
    int32_t n_imu;
    int32_t nq;                         /* rows of q: the range of seg_q_index */
    const double * kp;                  /* [n_imu] */
    const double * ki;                  /* [n_imu] */
    const double * rel_quat;            /* [n_imu][4] */
    const int32_t * frame_seg_start;    /* [n_imu + 1], ascending, last = n_seg */
    int32_t n_seg;
    const int32_t * seg_kind;           /* [n_seg] */
    const int32_t * seg_q_index;        /* [n_seg], -1 where seg_kind is 0 */
    const double * seg_rot;             /* [n_seg][9] */
    const double * seg_axis;            /* [n_seg][3] */
} jm_attitude_desc;
typedef struct jm_attitude_plan jm_attitude_plan;
int32_t jm_attitude_plan_create(const jm_attitude_desc * desc, jm_attitude_plan ** out);
int32_t jm_attitude_plan_destroy(jm_attitude_plan * plan);
int32_t jm_block_attitude_init(const jm_attitude_plan * plan, int32_t dtype, int64_t batch_size, const void * q,
                               const void * imu, const uint8_t * lane_mask, int32_t exact_init, void * quat, void * omega,
                               void * cf, void * bias, void * twist, void * rpy, void * stream);
int32_t jm_block_mahony_observer(const jm_attitude_plan * plan, int32_t dtype, int64_t batch_size, const void * imu,
                                 void * quat, void * omega, void * cf, void * bias, double dt, int32_t ignore_twist,
                                 void * rpy, void * stream);
int32_t jm_block_body_observer(const jm_attitude_plan * plan, int32_t dtype, int64_t batch_size, const void * imu_quat,
                               const void * imu_omega, void * quat, void * omega, void * twist, int32_t twist_mode,
                               double time_constant_inv, double dt, void * rpy, void * stream);

/* ---- Frame kinematics: pose and velocity of named frames from `q`, `v` (what the reference reads from `pinocchio_data.oMf`
 * and `getFrameVelocity`), and the SE3 step average of its quantity layer; batched, one lane = one environment.  New symbols
 * only: no existing structure or signature changed with them.
 * jm_frames_desc: the plan (host arrays, copied by jm_frames_plan_create).  Per frame a reference frame `frame_mode` (0 LOCAL,
 *   1 LOCAL_WORLD_ALIGNED, 2 ODOMETRY: the step average only, the velocity of such a frame is LOCAL) and the walk from the
 *   universe to the frame as a list of segments `frame_seg_start[f] .. frame_seg_start[f + 1] - 1`, at most 256 per frame: a
 *   segment is a constant placement (`seg_rot` row-major 3x3, `seg_trans`) followed by the motion of joint `seg_joint` read
 *   from `q` `[nq][B]` at `seg_q_index` and `v` `[nv][B]` at `seg_v_index`: `seg_kind` 0 none (the frame's own placement),
 *   1 / 2 / 3 revolute about x / y / z, 4 revolute about the unit vector `seg_axis`, 5 unbounded revolute about `seg_axis`
 *   with `(cos, sin) = q[i], q[i + 1]`, 6 spherical (unit quaternion `q[i .. i + 3]` xyzw, angular velocity `v[i .. i + 2]` in
 *   the joint frame), 7 free-flyer (`q`: position 3, quaternion 4; `v`: linear 3, angular 3, both local), 8 / 9 / 10
 *   prismatic along x / y / z, 11 prismatic along `seg_axis`.  The placement of a segment with a joint is the placement of
 *   that joint alone, so that `model_lane` can replace its translation.  jm_frames_plan_create validates the description
 *   (JM_EINVAL + jm_last_error, before any device call: null arrays, sizes, segment counts, `q` / `v` rows, joint indices in
 *   `[0, njoints)`, kinds, modes, finite constants) and uploads it; the two calls then allocate, copy and synchronise nothing.
 * jm_block_frame_kinematics: on the lanes of `lane_mask` (device, uint8 `[B]`; NULL: every lane; other lanes are not
 *   touched) writes, each or NULL, `pose` `[7][K][B]` (x y z, quaternion xyzw by the `matrices_to_quat` rule), `pose_prev`
 *   `[7][K][B]` (the same pose: the reset of the step average), `rpy` `[3][K][B]` (`quat_to_rpy`) and `vel` `[6][K][B]`
 *   (linear, angular, in the convention of pinocchio's `getFrameVelocity`: LOCAL `(R^T pdot, R^T omega)`, LOCAL_WORLD_ALIGNED
 *   `(pdot, omega)`, pdot the velocity of the frame origin; needs `v`).  `model_lane` (JM_F_MODEL_LANE `[13 * njoints][B]`,
 *   or NULL): the translation of the placement of joint j is rows `13 j + 10 .. 13 j + 12` of the lane.
 *   ≙ `FramePosition`, `FrameOrientation`, `FrameXYZQuat` (python/gym_jiminy/common/gym_jiminy/common/quantities/generic.py:298-950).
 * jm_block_frame_average: per lane and frame `diff = xyzquat_difference(pose_prev, pose)` (utils/math.py:1009-1042, with
 *   `log6` :842-894 and `log3` :725-774), `pose_mean = pose * exp6(-diff / 2)` (`exp6` :908-954, `exp3` :791-825;
 *   `AverageFrameXYZQuat`, generic.py:1357-1360), `quat_no_yaw = remove_yaw_from_quat(quaternion of pose_mean)` (:1148-1198;
 *   `AverageFrameRollPitch`), `v_avg = diff * inv_step_dt` with both halves rotated by nothing (LOCAL), the mean quaternion
 *   (LOCAL_WORLD_ALIGNED, generic.py:1522-1534) or `quat_no_yaw` (ODOMETRY, quantities/locomotion.py:281-288); last `pose` is
 *   copied into `pose_prev`.  `v_avg` `[6][K][B]`, `pose_mean` `[7][K][B]`, `quat_no_yaw` `[4][K][B]`, each or NULL.  The clamps
 *   of the divisions are `tiny` of the kernel's own scalar type: two identical poses give a zero difference and an
 *   unchanged mean in float32 as well.  `pose_prev` must not alias `pose`. */
typedef struct jm_frames_desc
{
    int32_t n_frames;
    int32_t nq;                         /* rows of q: the range of seg_q_index */
    int32_t nv;                         /* rows of v: the range of seg_v_index */
    int32_t njoints;                    /* the range of seg_joint */
    const int32_t * frame_seg_start;    /* [n_frames + 1], ascending, last = n_seg */
    const int32_t * frame_mode;         /* [n_frames] */
    int32_t n_seg;
    const int32_t * seg_kind;           /* [n_seg] */
    const int32_t * seg_joint;          /* [n_seg], -1 where seg_kind is 0 */
    const int32_t * seg_q_index;        /* [n_seg], -1 where seg_kind is 0 */
    const int32_t * seg_v_index;        /* [n_seg], -1 where seg_kind is 0 */
    const double * seg_rot;             /* [n_seg][9] */
    const double * seg_trans;           /* [n_seg][3] */
    const double * seg_axis;            /* [n_seg][3] */
} jm_frames_desc;
typedef struct jm_frames_plan jm_frames_plan;
int32_t jm_frames_plan_create(const jm_frames_desc * desc, jm_frames_plan ** out);
int32_t jm_frames_plan_destroy(jm_frames_plan * plan);
int32_t jm_block_frame_kinematics(const jm_frames_plan * plan, int32_t dtype, int64_t batch_size, const void * q,
                                  const void * v, const void * model_lane, const uint8_t * lane_mask, void * pose,
                                  void * pose_prev, void * rpy, void * vel, void * stream);
int32_t jm_block_frame_average(const jm_frames_plan * plan, int32_t dtype, int64_t batch_size, void * pose_prev,
                               const void * pose, double inv_step_dt, void * v_avg, void * pose_mean, void * quat_no_yaw,
                               void * stream);

/* ---- Locomotion quantities: what a locomotion learner shapes rewards and terminations with, from what a step left in
 * device memory; batched, one lane = one environment, one launch per refresh.  New symbols only: no existing structure or
 * signature changed with them.  Reference: python/gym_jiminy/common/gym_jiminy/common/quantities/locomotion.py and
 * compositions/locomotion.py, restated operation for operation.
 * jm_locomotion_desc: the plan (host arrays, copied by jm_locomotion_plan_create).  `body_mass` of every joint (joint 0, the
 *   universe, is not counted), the rotational inertia of the body of joint 1 in the order of JM_F_MODEL_LANE, `gravity` =
 *   |gravity_z|, `omega` = the natural frequency of `CapturePoint.initialize` (quantities/locomotion.py:1097-1112:
 *   sqrt(gravity / (com_z - lowest contact frame z)) at the neutral configuration), per contact point the foot it belongs to
 *   (`contact_foot`, -1: none; the contacts of one foot must be consecutive, :1440-1449) and the column of its frame in the
 *   tensors of the frame kinematics block (`contact_column`), the column of the root joint's frame (`root_column`), the
 *   number of columns `n_frames` (the row stride of those tensors is `n_frames * B`), and the reference frame of the ZMP and
 *   of the DCM (0 LOCAL = the odometry frame, 1 LOCAL_WORLD_ALIGNED).  jm_locomotion_plan_create validates the description
 *   (JM_EINVAL + jm_last_error, before any device call: null arrays, sizes, masses, finite constants, positive gravity and
 *   omega, reference frames, columns, foot indices, consecutive contacts, every foot with a contact) and uploads it; the
 *   launch then allocates, copies and synchronises nothing.
 * jm_locomotion_io: the device pointers of one launch, arrays `[rows][B]` of the scalar type `dtype`.  Every pointer may be
 *   NULL: the outputs that need it are then not written.  Inputs: `centroidal` `[15][B]` (JM_F_CENTROIDAL); `q_root` the
 *   first of the 7 root pose rows of `q`; `model_lane` (JM_F_MODEL_LANE `[13 * njoints][B]`: the mass of the robot is then
 *   the sum of the lane's mass rows of joints 1 .. njoints - 1 and the root inertia the lane's); `con_lambda` the first
 *   contact multiplier row of JM_F_CON_DATA (`[4 * n_contacts][B]`, behind the reference configurations and multipliers of
 *   the bounds); `con_flags` the first contact row of JM_F_CON_FLAGS (int32 `[n_contacts][B]`; a contact whose bit 0 is clear
 *   contributes zero, whatever its multiplier rows hold); `v_avg` `[6][K][B]`, `quat_no_yaw` `[4][K][B]`, `pose` `[7][K][B]`
 *   of the frame kinematics block, K = n_frames (the root column of `v_avg` must be a LOCAL frame); `lane_mask` (uint8 `[B]`,
 *   NULL: every lane; other lanes are not touched).  Outputs:
 *     com[3], vcom[3]          `CenterOfMass` (:814-887); vcom = hg_linear / mass (core/src/engine/engine.cc:896)
 *     odom_pose[3]             `BaseOdometryPose` (:158-219): x, y, atan2(sin_yaw, cos_yaw) of `quat_to_yaw_cos_sin`
 *                              (utils/math.py:95-141)
 *     zmp[2]                   `ZeroMomentPoint` (:914-1017): the NaN pair when |dhg_linear_z + weight| < float32 eps, in both
 *                              scalar types; `translate_position_odom` (:891-910) for LOCAL
 *     dcm[2]                   `CapturePoint` (:1021-1124)
 *     h_angular[3]             `AverageBaseMomentum` (:344-412): root inertia times the angular half of the root's LOCAL
 *                              `v_avg`, rotated by its `quat_no_yaw` (`quat_apply`, utils/math.py:645-709)
 *     contact_force_rel[6][n_contacts]   `MultiContactNormalizedSpatialForce` (:1128-1268): rows 0-2 and 5 the multipliers over
 *                              the weight, rows 3-4 zero
 *     foot_force_vertical[n_feet]        `MultiFootNormalizedForceVertical` (:1272-1481) on flat ground (the vertical
 *                              transform of every contact is e_z)
 *     scalars[4]               0 force_vertical_max: the largest row 2 of contact_force_rel (`ImpactForceTermination`,
 *                              compositions/locomotion.py:582-620); 1 ground_distance_min: `min_depth` on flat ground, the
 *                              lowest contact frame z (`FlyingTermination`, :450-579); 2 reward_momentum =
 *                              `radial_basis_function(h_angular, momentum_cutoff, 2)` (`MinimizeAngularMomentumReward`,
 *                              :257-281; compositions/mixin.py:17-66, CUTOFF_ESP = 1e-2); 3 reward_friction = the same of
 *                              rows 0-1 of contact_force_rel with `friction_cutoff` (`MinimizeFrictionReward`, :284-315).
 *                              A non-positive cutoff: that row is not written. */
typedef struct jm_locomotion_desc
{
    int32_t njoints;
    const double * body_mass;           /* [njoints] */
    const double * root_inertia;        /* [6] xx xy xz yy yz zz */
    double gravity;
    double omega;
    int32_t n_contacts;
    int32_t n_feet;
    const int32_t * contact_foot;       /* [n_contacts], -1: no foot */
    const int32_t * contact_column;     /* [n_contacts] */
    int32_t n_frames;
    int32_t root_column;
    int32_t zmp_frame;
    int32_t dcm_frame;
} jm_locomotion_desc;
typedef struct jm_locomotion_io
{
    const void * centroidal;
    const void * q_root;
    const void * model_lane;
    const void * con_lambda;
    const int32_t * con_flags;
    const void * v_avg;
    const void * quat_no_yaw;
    const void * pose;
    const uint8_t * lane_mask;
    void * com;
    void * vcom;
    void * odom_pose;
    void * zmp;
    void * dcm;
    void * h_angular;
    void * contact_force_rel;
    void * foot_force_vertical;
    void * scalars;
} jm_locomotion_io;
typedef struct jm_locomotion_plan jm_locomotion_plan;
int32_t jm_locomotion_plan_create(const jm_locomotion_desc * desc, jm_locomotion_plan ** out);
int32_t jm_locomotion_plan_destroy(jm_locomotion_plan * plan);
int32_t jm_block_locomotion(const jm_locomotion_plan * plan, int32_t dtype, int64_t batch_size, const jm_locomotion_io * io,
                            double momentum_cutoff, double friction_cutoff, void * stream);

/* ---- Locomotion quantities on height-map ground: jm_block_locomotion with the ground of jm_batch_set_ground under the
 * contact points, for the constraint contact model, whose contact rows live in the local frame [t0 t1 n] of the surface
 * under each contact point (FrameConstraint::setNormal, core/src/constraints/frame_constraint.cc:62-68).  New symbols only:
 * no existing structure or signature changed with them.
 * jm_locomotion_ground: `heights` the device array `[ny][nx]` of the scalar type `dtype`, sample (iy, ix) at (x0 + ix dx,
 *   y0 + iy dy), bilinear patches with flat continuation outside (the definition of jm_batch_set_ground); `offsets` `[2][B]`
 *   or NULL: the lane's (x, y) offset of every query (JM_F_GROUND_OFFSET); `contact_ground` `[4][n_contacts][B]` or NULL, an
 *   output: the height and the unit normal (x, y, z) of the ground under every contact point.
 * jm_block_locomotion_ground: `ground` NULL or `heights` NULL is flat ground: the kernel of jm_block_locomotion is launched,
 *   every output of `io` equals its bit for bit (`contact_ground`, where given, is then height 0 and normal e_z, written by a
 *   second small launch).  Otherwise, for every contact point, the world position
 *   of its frame (`io->pose`, required) plus the lane's offset is queried for the height h and the normal n, and
 *     foot_force_vertical[n_feet]   `MultiFootNormalizedForceVertical` (quantities/locomotion.py:1272-1481): per contact
 *                              t0_z lambda_x + t1_z lambda_y + n_z lambda_z, the third row of the constraint's `local_rotation`
 *                              on its multipliers, summed per foot, over the weight
 *     scalars[1]               ground_distance_min = min((z - h) n_z) (`_MultiContactMinGroundDistance`,
 *                              compositions/locomotion.py:449-540)
 *   Everything else is jm_block_locomotion's: `contact_force_rel`, scalars[0] and the friction reward stay in the local
 *   contact frame, as in the reference; the ZMP, the DCM, the CoM and the momentum do not look at the ground.  Validated
 *   before any device call (JM_EINVAL + jm_last_error): the arguments of jm_block_locomotion, nx < 2, ny < 2, a non-finite
 *   x0 / y0, a non-positive or non-finite dx / dy, a height map without `io->pose`.  The launch allocates, copies and
 *   synchronises nothing. */
typedef struct jm_locomotion_ground
{
    const void * heights;
    int32_t nx;
    int32_t ny;
    double x0;
    double y0;
    double dx;
    double dy;
    const void * offsets;
    void * contact_ground;
} jm_locomotion_ground;
int32_t jm_block_locomotion_ground(const jm_locomotion_plan * plan, int32_t dtype, int64_t batch_size, const jm_locomotion_io * io,
                                   const jm_locomotion_ground * ground, double momentum_cutoff, double friction_cutoff,
                                   void * stream);

/* ---- Actuated-joint quantities: kinematics of the actuated joints in motor order, distances to the mechanical stops, the
 * mechanical-safety count, the mechanical power, its sliding average over environment steps and the reward on it; batched,
 * one lane = one environment, one launch per refresh.  New symbols only: no existing structure or signature changed with
 * them.  Reference: python/gym_jiminy/common/gym_jiminy/common/quantities/generic.py:1538-1887 and
 * compositions/generic.py:153-191, 456-661, restated operation for operation.
 * jm_actuation_desc: the plan (host arrays, copied by jm_actuation_plan_create).  Per motor, in motor order: the row of its
 *   joint in `q` (`idx_q`) and in `v` / `a` (`idx_v`), its mechanical reduction (`MultiActuatedJointKinematic.initialize`,
 *   quantities/generic.py:1626-1645) and the position bounds of that row (`_MultiActuatedJointBoundDistance.initialize`,
 *   compositions/generic.py:486-498); `nq` / `nv` the rows of `q` / `v`; `generator_mode` the `EnergyGenerationMode`
 *   (quantities/generic.py:1694-1719: 0 CHARGE, 1 LOST_EACH, 2 LOST_GLOBAL, 3 PENALIZE); `max_stack` the length of the sliding
 *   window (`AverageMechanicalPowerConsumption.__init__`, :1865: max(ceil(horizon / step_dt), 1) + 1).
 *   jm_actuation_plan_create validates the description (JM_EINVAL + jm_last_error, before any device call: null arrays,
 *   1 <= n_motors <= 256, indices inside nq / nv, finite reductions and bounds, low <= high, the generator mode,
 *   2 <= max_stack <= 1024) and uploads it; the launch then allocates, copies and synchronises nothing.
 * jm_actuation_io: the device pointers of one launch, arrays `[rows][B]` of the scalar type `dtype` but the three integer
 *   ones.  Every pointer may be NULL: the outputs that need it are then not written.  Inputs: `q` `[nq][B]`, `v`, `a`
 *   `[nv][B]`, `command` `[n_motors][B]` (the motor efforts), `lane_mask` (uint8 `[B]`, NULL: every lane; other lanes are
 *   not touched).  State, owned by the caller: `power_ring` `[max_stack][B]`, `power_count` (int32 `[B]`, the `num_steps` of
 *   the reference's stack per lane).  Outputs, each in motor order:
 *     position, velocity, acceleration [n_motors]   `MultiActuatedJointKinematic.refresh` (quantities/generic.py:1675-1691):
 *                              the row of the state, times the reduction when `motor_side` is non-zero (one flag for the
 *                              three levels)
 *     bound_low, bound_high [n_motors]   `_MultiActuatedJointBoundDistance.refresh` (compositions/generic.py:500-502):
 *                              position - low, high - position on the joint side, whatever `motor_side`
 *     safety (int32 [B])       the number of motors with (bound_low < position_margin) & (v < -velocity_max) or
 *                              (bound_high < position_margin) & (v > velocity_max), v on the joint side
 *                              (`MechanicalSafetyTermination.compute`, :585-595: it terminates when the count is not
 *                              zero).  A negative `velocity_max`: not written.
 *     scalars[3]               0 power: `compute_power` (quantities/generic.py:1723-1746) of `command` and v * reduction;
 *                              1 power_average: `AverageMechanicalPowerConsumption.refresh` (:1886-1887), `np.sum / size` over
 *                              the wrapping stack of `StackedQuantity.refresh` (quantities/transform.py:208-296); 2
 *                              reward_power = `radial_basis_function(power_average, power_cutoff, 2)`
 *                              (`MinimizeMechanicalPowerConsumption`, compositions/generic.py:153-191).  A non-positive
 *                              cutoff: row 2 is not written; without the ring or the counter: rows 1-2 are not written.
 * jm_block_actuation: `mode` 0 restarts the window of the launched lanes (count = 0, slot 0 = the current power, the average
 *   is that value: what the first refresh of an episode gives), `mode` 1 pushes (count += 1, slot count % max_stack = the
 *   current power, the average over the first min(count + 1, max_stack) slots in storage order).  No argument changes from
 *   step to step, so the launch can be part of a captured graph. */
typedef struct jm_actuation_desc
{
    int32_t n_motors;
    int32_t nq;
    int32_t nv;
    const int32_t * idx_q;              /* [n_motors] */
    const int32_t * idx_v;              /* [n_motors] */
    const double * reduction;           /* [n_motors] */
    const double * position_low;        /* [n_motors] */
    const double * position_high;       /* [n_motors] */
    int32_t generator_mode;
    int32_t max_stack;
} jm_actuation_desc;
typedef struct jm_actuation_io
{
    const void * q;
    const void * v;
    const void * a;
    const void * command;
    const uint8_t * lane_mask;
    void * position;
    void * velocity;
    void * acceleration;
    void * bound_low;
    void * bound_high;
    int32_t * safety;
    void * scalars;
    void * power_ring;
    int32_t * power_count;
} jm_actuation_io;
typedef struct jm_actuation_plan jm_actuation_plan;
int32_t jm_actuation_plan_create(const jm_actuation_desc * desc, jm_actuation_plan ** out);
int32_t jm_actuation_plan_destroy(jm_actuation_plan * plan);
int32_t jm_block_actuation(const jm_actuation_plan * plan, int32_t dtype, int64_t batch_size, const jm_actuation_io * io,
                           int32_t mode, int32_t motor_side, double position_margin, double velocity_max, double power_cutoff,
                           void * stream);

/* ---- Foot pose quantities: the mean pose of the feet of a legged robot, its odometry pose, the pose of every foot but the
 * last relative to the mean, and the tracking error and rewards against a reference of the relative poses; batched, one
 * lane = one environment, one launch per refresh.  New symbols only: no existing structure or signature changed with them.
 * Reference: python/gym_jiminy/common/gym_jiminy/common/quantities/generic.py:950-1062, quantities/locomotion.py:416-557 and
 * :683-810, compositions/generic.py:64-122, compositions/locomotion.py:146-214, restated operation for operation.
 * jm_footposes_desc: the plan (host array, copied by jm_footposes_plan_create).  `n_frames` = K, the number of columns of the
 *   `pose` tensor of the frame kinematics block (its row stride is `n_frames * B`); per foot, in the order of
 *   `sanitize_foot_frame_names` (quantities/locomotion.py:31-84: sorted names), the column of its frame (`foot_column`).
 *   jm_footposes_plan_create validates the description (JM_EINVAL + jm_last_error, before any device call: null array,
 *   1 <= n_feet <= 64, n_feet <= n_frames, columns inside [0, n_frames), no column twice) and uploads it; the launch then
 *   allocates, copies and synchronises nothing.
 * jm_footposes_io: the device pointers of one launch, arrays `[rows][B]` of the scalar type `dtype`, F = n_feet.  Every
 *   pointer may be NULL: the outputs that need it are then not written.  Inputs: `pose` `[7][K][B]` (x y z, quaternion xyzw);
 *   `reference_relative_pose` `[7][F - 1][B]`, the reference value of `relative_pose` (what `QuantityEvalMode.REFERENCE` gives
 *   the reference's tracking rewards); `lane_mask` (uint8 `[B]`, NULL: every lane; other lanes are not touched).  Outputs:
 *     mean_pose[7]             `MultiFootMeanXYZQuat` (quantities/locomotion.py:416-478) = `MultiFrameMeanXYZQuat.refresh`
 *                              (quantities/generic.py:1055-1062): `position_average` and `quat_average_2d` (:950-980) -- one
 *                              foot: a copy; two: `quat_interpolate_middle` (utils/math.py:1296-1331); three or more: the
 *                              eigenvector of the largest eigenvalue of sum q q^T, with a non-negative dot product with the
 *                              first foot's quaternion (LAPACK's sign, which the reference inherits, is arbitrary)
 *     mean_odom_pose[3]        `MultiFootMeanOdometryPose` (quantities/locomotion.py:482-557): x, y of the mean, `quat_to_yaw`
 *                              (utils/math.py:95-141) of its quaternion
 *     relative_pose[7][F - 1]  `MultiFootRelativeXYZQuat.refresh` (:779-810): R_mean^T (p_i - p_mean) (`quat_to_matrix`,
 *                              utils/math.py:214-248; `translate_positions`, :683-698) and conj(q_mean) q_i (`quat_multiply`,
 *                              utils/math.py:570-626), the last foot dropped
 *     tracking_error[6][F - 1] with a reference only: rows 0-2 relative position - reference position, rows 3-5
 *                              `quat_difference(relative quaternion, reference quaternion)` (utils/math.py:971-1005, `log3`
 *                              :724-774): the errors `TrackingQuantityReward` (compositions/generic.py:64-122) feeds its kernel
 *     scalars[2]               0 reward_foot_positions = `radial_basis_function(rows 0-2, position_cutoff, 2)`
 *                              (`TrackingFootPositionsReward`, compositions/locomotion.py:146-176; compositions/mixin.py:17-66,
 *                              CUTOFF_ESP = 1e-2); 1 reward_foot_orientations = the same of rows 3-5 with `orientation_cutoff`
 *                              (`TrackingFootOrientationsReward`, :179-214).  A non-positive cutoff: that row is not written;
 *                              without a reference neither is, unless F = 1, where the error is empty and both are 1. */
typedef struct jm_footposes_desc
{
    int32_t n_frames;
    int32_t n_feet;
    const int32_t * foot_column;        /* [n_feet] */
} jm_footposes_desc;
typedef struct jm_footposes_io
{
    const void * pose;
    const void * reference_relative_pose;
    const uint8_t * lane_mask;
    void * mean_pose;
    void * mean_odom_pose;
    void * relative_pose;
    void * tracking_error;
    void * scalars;
} jm_footposes_io;
typedef struct jm_footposes_plan jm_footposes_plan;
int32_t jm_footposes_plan_create(const jm_footposes_desc * desc, jm_footposes_plan ** out);
int32_t jm_footposes_plan_destroy(jm_footposes_plan * plan);
int32_t jm_block_foot_poses(const jm_footposes_plan * plan, int32_t dtype, int64_t batch_size, const jm_footposes_io * io,
                            double position_cutoff, double orientation_cutoff, void * stream);

/* ---- Tracking windows: the drift of the base odometry pose and the shift of the relative foot poses and of the motor
 * positions against a reference motion, each over a sliding window of environment steps; batched, one lane = one
 * environment, one launch per refresh.  New symbols only: no existing structure or signature changed with them.  Reference:
 * python/gym_jiminy/common/gym_jiminy/common/quantities/transform.py:208-296 (`StackedQuantity.refresh`, both branches) and
 * :715-831 (`DeltaQuantity`), quantities/locomotion.py:1537-1693, compositions/generic.py:194-453 and :664-716,
 * compositions/locomotion.py:76-120 and :623-867, restated operation for operation.
 * jm_tracking_desc: the plan.  One window length per family, `max(ceil(horizon / step_dt), 1) + 1` (compositions/generic.py:430,
 *   quantities/locomotion.py:1573), 0: the family is absent; `n_rel` = F - 1, the columns of the relative foot poses; `n_motors`
 *   the rows of the motor positions.  jm_tracking_plan_create validates the description (JM_EINVAL + jm_last_error, before any
 *   device call: 2 <= each max_stack <= 1024, 1 <= n_rel <= 63, 1 <= n_motors <= 256, the sizes of an absent family 0, at least
 *   one family) and uploads it; the launch then allocates, copies and synchronises nothing.
 * jm_tracking_io: the device pointers of one launch, arrays `[rows][B]` of the scalar type `dtype` but the two integer ones.
 *   Every pointer may be NULL: a family one of whose inputs or state arrays is NULL is skipped, an output that is NULL is not
 *   written; without `count` nothing runs.  Inputs: `odom_pose`, `reference_odom_pose` `[3][B]` (x, y, yaw: `BaseOdometryPose`);
 *   `relative_pose`, `reference_relative_pose` `[7][n_rel][B]` (`MultiFootRelativeXYZQuat`); `position`, `reference_position`
 *   `[n_motors][B]` (`MultiActuatedJointKinematic`, joint side); `lane_mask` (uint8 `[B]`, NULL: every lane; other lanes are
 *   not touched).  State, owned by the caller: `count` (int32 `[B]`, the `num_steps` of the reference's stacks per lane, shared
 *   by the families); `odom_ring` `[max_stack_odom][4][B]` (true x, true y, reference x, reference y), `yaw_prev` `[2][B]`,
 *   `yaw_ring` `[max_stack_odom - 1][2][B]` (true, reference); `foot_ring` `[2][max_stack_foot][B]`; `motor_ring`
 *   `[max_stack_motor][B]`.  Outputs:
 *     delta_odom, delta_odom_reference [3]   `DeltaBaseOdometryPosition` (quantities/locomotion.py:1537-1599: newest - oldest
 *                              value of the window, `DeltaQuantity` with bounds_only=True) and `DeltaBaseOdometryOrientation`
 *                              (:1630-1693: the sum over the window of `angle_difference` (:1602-1627) between successive steps,
 *                              bounds_only=False, so that turns are counted), of the true and of the reference pose
 *     scalars[6]               0 drift_odom_position = |dxy_true - dxy_ref|, 1 drift_odom_orientation = |dyaw_true - dyaw_ref|
 *                              (`compute_drift_error`, compositions/generic.py:194-208;
 *                              `DriftTrackingBaseOdometryPositionTermination` / `...OrientationTermination`,
 *                              compositions/locomotion.py:623-736); 2 reward_odom_pose = `radial_basis_function([|dxy_true| -
 *                              |dxy_ref|, dyaw_true - dyaw_ref], odometry_cutoff, 2)` (`DriftTrackingBaseOdometryPoseReward`,
 *                              :85-120; a non-positive cutoff: not written); 3 shift_foot_positions, 4
 *                              shift_foot_orientations: `min_norm` (compositions/generic.py:318-330) over the window of the
 *                              difference of rows 0-1, and of `angle_distance` (compositions/locomotion.py:794-810) of the
 *                              `quat_to_yaw` (utils/math.py:95-141) of rows 3-6, of the relative foot poses
 *                              (`ShiftTrackingFootOdometryPositionsTermination` / `...OrientationsTermination`, :739-867); 5
 *                              shift_motor_positions: `min_norm` of position - reference
 *                              (`ShiftTrackingMotorPositionsTermination`, compositions/generic.py:664-716).  The rings of the
 *                              two shift families hold one sum of squares per timestamp, which `min_norm` reduces.  NaN
 *                              propagates like `np.min` and `np.sum`.
 * jm_block_tracking: `mode` 0 restarts the windows of the launched lanes (count = 0: what the first refresh of an episode
 *   gives), `mode` 1 pushes one environment step (count += 1).  No argument changes from step to step, so the launch can be part
 *   of a captured graph. */
typedef struct jm_tracking_desc
{
    int32_t max_stack_odom;
    int32_t max_stack_foot;
    int32_t max_stack_motor;
    int32_t n_rel;
    int32_t n_motors;
} jm_tracking_desc;
typedef struct jm_tracking_io
{
    const void * odom_pose;
    const void * reference_odom_pose;
    const void * relative_pose;
    const void * reference_relative_pose;
    const void * position;
    const void * reference_position;
    const uint8_t * lane_mask;
    int32_t * count;
    void * odom_ring;
    void * yaw_prev;
    void * yaw_ring;
    void * foot_ring;
    void * motor_ring;
    void * delta_odom;
    void * delta_odom_reference;
    void * scalars;
} jm_tracking_io;
typedef struct jm_tracking_plan jm_tracking_plan;
int32_t jm_tracking_plan_create(const jm_tracking_desc * desc, jm_tracking_plan ** out);
int32_t jm_tracking_plan_destroy(jm_tracking_plan * plan);
int32_t jm_block_tracking(const jm_tracking_plan * plan, int32_t dtype, int64_t batch_size, const jm_tracking_io * io, int32_t mode,
                          double odometry_cutoff, void * stream);

/* ---- Reference trajectories: a device-resident dataset of recorded trajectories and the state of each lane's selected
 * trajectory at the lane's own time -- what `QuantityEvalMode.REFERENCE` reads; batched, one lane = one environment, one
 * launch per query.  New symbols only: no existing structure or signature changed with them.  Reference:
 * python/jiminy_py/src/jiminy_py/dynamics.py:296-388 (`Trajectory.get`: the time mode, `bisect_left`, the choice of a sample
 * or `alpha`, `pin.interpolate` of `q`, the linear interpolation of the other fields, the odometry of a wrapping time),
 * :207-213 (the stride), :31 (`TRAJ_INTERP_TOL`); python/gym_jiminy/common/gym_jiminy/common/bases/quantities.py:870-1210
 * (`DatasetTrajectoryQuantity`: the registry, the selection and the time offset, `lock`); utils/math.py:725-954 (`log3`, `exp3`,
 * `log6`, `exp6`); quantities/locomotion.py:158-220 (`BaseOdometryPose`), restated operation for operation.
 * jm_trajectory_desc: the dataset and the layout of `q`.  `n_trajectories` trajectories concatenated along the sample axis:
 *   `sample_start[n_trajectories + 1]` (from 0 to `n_samples`, at least 2 samples each), `times[n_samples]` (float64, finite,
 *   not decreasing inside a trajectory; two equal consecutive times are t-, t+), `mode[n_trajectories]` (0 raise, 1 wrap,
 *   2 clip), `stride[n_trajectories][6]` (float64, `log6(M_end * M_start^-1)` of the free-flyer, linear then angular; read
 *   only with a free-flyer, NULL without one), `data[n_samples][R]` (HOST memory, scalar type `dtype`, sample-major; a row is
 *   q (nq), then v (nv) with `fields` bit 0, a (nv) with bit 1, command (n_command) with bit 2).  The joint table: per joint its
 *   kind (1-4 revolute, 5 unbounded revolute: cos, sin; 6 spherical: quaternion xyzw; 7 free-flyer: position, quaternion; 8-11
 *   prismatic -- the kinds of jm_frames_desc) and its first row of `q`; a free-flyer is joint 0 at row 0.  `motor_q_index
 *   [n_motors]`: the `q` rows of the motors, each the row of a one-row joint.  jm_trajectory_plan_create validates all of it
 *   (JM_EINVAL + jm_last_error naming the entry, before any device call) and copies the tables and the samples to the device;
 *   the plan is immutable afterwards.
 * jm_trajectory_io: the device pointers of one launch.  Inputs: `time` (float64 `[B]`, the lane's episode time), `trajectory`
 *   (int32 `[B]`), `time_offset` (float64 `[B]`), `lane_mask` (uint8 `[B]`, NULL: every lane; other lanes are not touched).
 *   Outputs `[rows][B]` of the scalar type, each may be NULL: `q [nq]`, `v`, `a` `[nv]`, `command [n_command]` (absent fields
 *   are never written), `odom_pose [3]` (x, y, yaw of the free-flyer, the expression of jm_block_locomotion; free-flyer only),
 *   `position [n_motors]` (`q[motor_q_index]`), `status` (int32 `[3][B]`: flags, `n_steps`, the right sample's index inside the
 *   trajectory).  Flags: bit 0 the query time is out of range in mode raise (the reference raises; the launch goes on with
 *   the clipped time), or is not finite; bit 1 `trajectory` is outside the dataset (nothing else is written for the lane).
 * jm_block_trajectory_state: the query time `time + time_offset`, the mode handling, the search and `alpha` are float64
 *   for both dtypes.  `dtype` must be the plan's.  No argument changes from step to step, so the launch can be part of a
 *   captured graph. */
typedef struct jm_trajectory_desc
{
    int32_t dtype;
    int32_t n_trajectories;
    int32_t n_samples;
    const int32_t * sample_start;
    const double * times;
    const int32_t * mode;
    const double * stride;
    int32_t nq;
    int32_t nv;
    int32_t n_command;
    int32_t fields;
    const void * data;
    int32_t n_joints;
    const int32_t * joint_kind;
    const int32_t * joint_q_index;
    int32_t n_motors;
    const int32_t * motor_q_index;
} jm_trajectory_desc;
typedef struct jm_trajectory_io
{
    const double * time;
    const int32_t * trajectory;
    const double * time_offset;
    const uint8_t * lane_mask;
    void * q;
    void * v;
    void * a;
    void * command;
    void * odom_pose;
    void * position;
    int32_t * status;
} jm_trajectory_io;
typedef struct jm_trajectory_plan jm_trajectory_plan;
int32_t jm_trajectory_plan_create(const jm_trajectory_desc * desc, jm_trajectory_plan ** out);
int32_t jm_trajectory_plan_destroy(jm_trajectory_plan * plan);
int32_t jm_block_trajectory_state(const jm_trajectory_plan * plan, int32_t dtype, int64_t batch_size, const jm_trajectory_io * io,
                                  void * stream);

/* ---- Centroidal quantities of an arbitrary state: the centre of mass, the centroidal momentum and its time derivative from
 * any `(q, v, a)` -- what the reference computes on the CPU with `pin.computeCentroidalMomentumTimeVariation`
 * (python/jiminy_py/src/jiminy_py/dynamics.py:496-499, reached from `StateQuantity.refresh`,
 * python/gym_jiminy/common/gym_jiminy/common/bases/quantities.py:1494-1518) for the state of a reference trajectory; batched,
 * one lane = one environment, one launch per call.  New symbols only: no existing structure or signature changed with them.
 * jm_centroidal_desc: the plan (host arrays, copied by jm_centroidal_plan_create) of the NOMINAL model.  Per body the walk from
 *   the universe to the body's joint frame as a list of segments `body_seg_start[b] .. body_seg_start[b + 1] - 1` in the tables
 *   of jm_frames_desc (kinds, rows, placements, axes; at most 256 per body), and its `body_mass`, `body_com` (in the joint frame)
 *   and `body_inertia` (about the centre of mass, joint-frame axes: xx xy xz yy yz zz).  jm_centroidal_plan_create validates the
 *   description like jm_frames_plan_create (JM_EINVAL + jm_last_error, before any device call) and also rejects constants
 *   that are not finite, a negative mass and a total mass that is not positive.  ≙ the inertias of `pinocchio_model`.
 * jm_block_centroidal_state: on the lanes of `lane_mask` (device, uint8 `[B]`; NULL: every lane; other lanes are not touched)
 *   writes `centroidal` `[15][B]` in the row layout of JM_F_CENTROIDAL: com (3), hg (6: linear then angular, about the centre
 *   of mass, world axes), dhg (6: `I a + v x* I v` summed over the bodies -- no gravity, no external forces, `fBody[0]` of
 *   `computeExtraTerms`, core/src/engine/engine.cc:800-905).  `q` `[nq][B]`, `v`, `a` `[nv][B]` in pinocchio's convention
 *   (spatial, in the joint's local frame); `a` may be NULL: the dhg rows are then written as zeros.  The centre-of-mass
 *   velocity is `hg_linear / mass`.  Allocates, copies and synchronises nothing; no argument changes from call to call, so
 *   the launch can be part of a captured graph. */
typedef struct jm_centroidal_desc
{
    int32_t n_bodies;
    int32_t nq;                         /* rows of q: the range of seg_q_index */
    int32_t nv;                         /* rows of v, a: the range of seg_v_index */
    int32_t njoints;                    /* the range of seg_joint */
    const int32_t * body_seg_start;     /* [n_bodies + 1], ascending, last = n_seg */
    int32_t n_seg;
    const int32_t * seg_kind;           /* [n_seg] */
    const int32_t * seg_joint;          /* [n_seg], -1 where seg_kind is 0 */
    const int32_t * seg_q_index;        /* [n_seg], -1 where seg_kind is 0 */
    const int32_t * seg_v_index;        /* [n_seg], -1 where seg_kind is 0 */
    const double * seg_rot;             /* [n_seg][9] */
    const double * seg_trans;           /* [n_seg][3] */
    const double * seg_axis;            /* [n_seg][3] */
    const double * body_mass;           /* [n_bodies] */
    const double * body_com;            /* [n_bodies][3] */
    const double * body_inertia;        /* [n_bodies][6] */
} jm_centroidal_desc;
typedef struct jm_centroidal_plan jm_centroidal_plan;
int32_t jm_centroidal_plan_create(const jm_centroidal_desc * desc, jm_centroidal_plan ** out);
int32_t jm_centroidal_plan_destroy(jm_centroidal_plan * plan);
int32_t jm_block_centroidal_state(const jm_centroidal_plan * plan, int32_t dtype, int64_t batch_size, const void * q,
                                  const void * v, const void * a, const uint8_t * lane_mask, void * centroidal, void * stream);

/* ---- Tracking rewards on balance quantities: a quantity on the true state and on the state of the reference trajectory, and
 * the radial basis function of their difference -- the `TrackingQuantityReward` family
 * (python/gym_jiminy/common/gym_jiminy/common/compositions/generic.py:64-122); batched, one lane = one environment, one launch per
 * refresh.  New symbols only: no existing structure or signature changed with them.  Terms, in the order of the rows of
 * `rewards` and of `cutoff`: 0 base height ≙ `TrackingBaseHeightReward` (compositions/locomotion.py:33-51; `compute_height`,
 * quantities/locomotion.py:88-97: root z minus the lowest contact frame z of `pose`); 1 odometry velocity ≙
 * `TrackingBaseOdometryVelocityReward` (:54-72; rows (0, 1, 5) of `quat_apply(quat_no_yaw, v_avg)` of the root column, which is
 * LOCAL: quantities/locomotion.py:281-288, :329-333); 2 capture point ≙ `TrackingCapturePointReward` (:123-143; the `dcm` of two
 * jm_block_locomotion launches, LOCAL); 3 joint positions ≙ `TrackingActuatedJointPositionsReward`
 * (compositions/generic.py:125-150).
 * jm_trackrewards_desc: the columns of 'root_joint' and of the contact frames in the tensors of the true and of the reference
 *   frame kinematics block (`n_frames`, `n_frames_reference` columns; 0: that side has none), and the number of motors.
 *   jm_trackrewards_plan_create validates it (JM_EINVAL + jm_last_error, before any device call).
 * jm_trackrewards_io: the device pointers of one launch, each or NULL.  Outputs: `value`, `reference` `[6 + n_motors][B]` (the
 *   true and the reference side concatenated: height 1, odometry velocity 3, capture point 2, joint positions n_motors),
 *   `rewards` `[4][B]` = `radial_basis_function(value - reference, cutoff, 2)` (compositions/mixin.py:26-66).
 * jm_block_tracking_rewards: `cutoff[4]` (host); a term whose cutoff is not positive or whose inputs are NULL is skipped and
 *   its rows are not written.  Lanes outside `lane_mask` (uint8 `[B]`, NULL: every lane) are not touched.  No argument
 *   changes from step to step, so the launch can be part of a captured graph. */
typedef struct jm_trackrewards_desc
{
    int32_t n_contacts;
    int32_t n_motors;
    int32_t n_frames;
    int32_t root_column;
    const int32_t * contact_column;             /* [n_contacts] */
    int32_t n_frames_reference;
    int32_t root_column_reference;
    const int32_t * contact_column_reference;   /* [n_contacts] */
} jm_trackrewards_desc;
typedef struct jm_trackrewards_io
{
    const void * pose;
    const void * pose_reference;
    const void * v_avg;
    const void * quat_no_yaw;
    const void * v_avg_reference;
    const void * quat_no_yaw_reference;
    const void * dcm;
    const void * dcm_reference;
    const void * position;
    const void * position_reference;
    const uint8_t * lane_mask;
    void * value;
    void * reference;
    void * rewards;
} jm_trackrewards_io;
typedef struct jm_trackrewards_plan jm_trackrewards_plan;
int32_t jm_trackrewards_plan_create(const jm_trackrewards_desc * desc, jm_trackrewards_plan ** out);
int32_t jm_trackrewards_plan_destroy(jm_trackrewards_plan * plan);
int32_t jm_block_tracking_rewards(const jm_trackrewards_plan * plan, int32_t dtype, int64_t batch_size, const jm_trackrewards_io * io,
                                  const double * cutoff, void * stream);

/* ---- Projected support polygon: the 2D convex hull of every candidate contact point of a legged robot, its barycenter, the
 * signed distance of the ZMP from its border and the robustness reward on it; batched, one lane = one environment, one
 * launch per refresh.  New symbols only: no existing structure or signature changed with them.  Reference:
 * python/gym_jiminy/toolbox/gym_jiminy/toolbox/math/qhull.py:52-224 and :396-457, quantities/locomotion.py:22-239,
 * compositions/locomotion.py:15-115, restated operation for operation (csrc/jm_support.h).  The reference's host-side pruning
 * of the contact points by the 3D hull of their body is not built: every point of the plan is a candidate.
 * jm_support_desc: the plan (host array, copied by jm_support_plan_create).  `n_frames` = K, the number of columns of the
 *   `pose` tensor of the frame kinematics block; per candidate point, in the model's contact order, the column of its frame
 *   (`point_column`); `reference_frame` 0 (LOCAL: every point goes through `translate_position_odom` with the lane's
 *   `odom_pose`) or 1 (LOCAL_WORLD_ALIGNED: the world coordinates as they are).  jm_support_plan_create validates the
 *   description (JM_EINVAL + jm_last_error, before any device call: null array, 1 <= n_points <= 16, n_points <= n_frames,
 *   columns inside [0, n_frames), no column twice, a frame other than the two) and uploads it; the launch then allocates,
 *   copies and synchronises nothing.
 * jm_support_io: the device pointers of one launch, arrays `[rows][B]` of the scalar type `dtype` (the two index outputs
 *   int32).  Every pointer may be NULL: the outputs that need it are then not written.  Inputs: `pose` `[7][K][B]` (rows 0
 *   and 1 are read); `odom_pose` `[3][B]` and `zmp` `[2][B]` of the locomotion quantities block, `zmp` in the plan's
 *   reference frame (LOCAL without `odom_pose`: nothing is written); `lane_mask` (uint8 `[B]`, NULL: every lane; other lanes
 *   are not touched).  Outputs:
 *     n_vertices               the number of vertices of the hull
 *     vertex_index[16]         their indices into `point_column`, in the reference's order (`compute_convex_hull_vertices`:
 *                              the sorted order itself with 3 points or fewer, else the upper chain then the lower chain); -1
 *                              from `n_vertices` on
 *     vertices[2][16]          their coordinates; NaN from `n_vertices` on
 *     center[2]                `ConvexHull2D.center`: the mean of the vertices
 *     scalars[2]               0 stability_margin = minus `ConvexHull2D.get_distance_to_point(zmp)`, -inf where `zmp[0]` is NaN
 *                              (`StabilityMarginProjectedSupportPolygon`); 1 reward_robustness = `sigmoid_normalization(margin,
 *                              -cutoff_outer, cutoff_inner, True)` (`MaximizeRobustness`), written where both cutoffs are
 *                              positive.  Without `zmp` neither row is written.
 * jm_block_support_polygon: a negative or non-finite cutoff is JM_EINVAL.  A lane whose inputs are NaN or infinite
 *   terminates like any other, with `n_vertices` in [0, 16], indices in [-1, n_points) and an arbitrary margin. */
typedef struct jm_support_desc
{
    int32_t n_frames;
    int32_t n_points;
    int32_t reference_frame;
    const int32_t * point_column;       /* [n_points] */
} jm_support_desc;
typedef struct jm_support_io
{
    const void * pose;
    const void * odom_pose;
    const void * zmp;
    const uint8_t * lane_mask;
    int32_t * n_vertices;
    int32_t * vertex_index;
    void * vertices;
    void * center;
    void * scalars;
} jm_support_io;
typedef struct jm_support_plan jm_support_plan;
int32_t jm_support_plan_create(const jm_support_desc * desc, jm_support_plan ** out);
int32_t jm_support_plan_destroy(jm_support_plan * plan);
int32_t jm_block_support_polygon(const jm_support_plan * plan, int32_t dtype, int64_t batch_size, const jm_support_io * io,
                                 double cutoff_inner, double cutoff_outer, void * stream);

/* ---- Composition layer: the termination conditions and the reward tree of `ComposedJiminyEnv(reward=..., terminations=[...])`
 * on the rows other blocks left on the device; batched, one lane = one environment, one launch per environment step,
 * independent of the topology.  New symbols only: no existing structure or signature changed with them.  Reference
 * (python/gym_jiminy/common/gym_jiminy/common): bases/compositions.py:88-663 (`AbstractReward.__call__`, `QuantityReward`,
 * `MixtureReward`, `AbstractTerminationCondition.__call__`, `QuantityTermination`), compositions/mixin.py:70-258
 * (`weighted_norm`, `geometric_mean` and the two mixtures), compositions/generic.py:32-61 (`SurviveReward`),
 * bases/pipeline.py:751-797 (`ComposedJiminyEnv.has_terminated`), utils/spaces.py:81-104 (`_array_contains`).
 * jm_compose_desc: the plan (host arrays, copied by jm_compose_plan_create, which validates them: JM_EINVAL + jm_last_error
 *   before any device call).
 *   Sources, at most 16: slot s is the base pointer `source[s]` of the launch, an array `[source_rows[s]][B]` of the element
 *     kind `source_kind[s]`: 0 the scalar type `dtype`, 1 int32, 2 uint8.  Every leaf and element is a (slot, row).
 *   Reward tree, at most 32 nodes and 4 levels; none: the reward is 0.  Node 0 is the root; a child has a larger index than
 *     its parent and exactly one parent.  `node_kind`: 0 leaf (`node_slot`, `node_row`), 1 `SurviveReward`, 2 additive mixture
 *     (`node_order`: p > 0 or infinity; the entries `node_child_start`, `node_child_count` of `child` / `child_weight`, every
 *     weight positive), 3 multiplicative mixture (weights not read).  `node_terminal`: 1 terminal, 0 non-terminal, -1
 *     indefinite; `node_normalized`: the node is advertised to stay in [0, 1].  Both are the caller's for every node (the
 *     reference's constructors derive those of a mixture: jiminy_amd.compositions does the same).
 *   Terminations, at most 16 conditions in evaluation order with at most 64 elements in total: condition c owns the elements
 *     `cond_elem_start[c]` .. + `cond_elem_count[c]`; `cond_flags`: 1 array form (a NaN element fires; without it the
 *     condition is the 0-d form, has one element, and NaN does not fire), 2 `is_truncation`, 4 `training_only`;
 *     `cond_grace`.  Element e reads (`elem_slot`, `elem_row`) and fires outside [`elem_low`, `elem_high`], each bound
 *     present by `elem_bounds` (1 low, 2 high).
 * jm_compose_io: the device pointers of one launch.  Inputs: `source[16]`; `time` `[B]` (scalar type; NULL: 0), the lane's
 *   episode time; `base_terminated`, `base_truncated` (uint8 `[B]`, NULL: 0), the flags of the environment below;
 *   `lane_mask` (uint8 `[B]`, NULL: every lane; other lanes are not touched).  Outputs, each or NULL:
 *     terminated, truncated    uint8 `[B]`.  A lane with a base flag keeps both flags as they are and evaluates no condition;
 *                              else the conditions run in order, condition c being skipped where it is `training_only` and
 *                              `training` is 0 or where `time < cond_grace[c]`; the first that fires sets `terminated`, or
 *                              `truncated` with `is_truncation`, and ends the loop
 *     trigger                  int32 `[B]`: that condition; -1 where none fired, or a base flag was set
 *     reward                   `[B]`: the value of node 0 with the `terminated` above; 0 where it is not evaluated
 *     node_value               `[n_nodes][B]`: the value of every evaluated node (the reference's `info`), NaN elsewhere.  A
 *                              node is evaluated where `(node_terminal == 1) == terminated` (an indefinite node counts as
 *                              non-terminal) and, a mixture, at least one child is; the reduction runs over the evaluated
 *                              children: `pow(sum w_i pow(v_i, p), 1 / p)`, the maximum of `w_i v_i` (which skips a NaN
 *                              behind the first child, like Python's `max`), or `pow(prod v_i, 1 / n)`
 *     violations               int32 `[B]`: bit n set for the first evaluated node n, in evaluation order (children before
 *                              their parent), that is advertised as normalised and left [0, 1], where the reference raises
 *                              ValueError; 0: none.  The values are written regardless.
 * jm_block_compose: `training` is the environment's mode of this launch, not part of the plan.  Nothing is allocated, copied
 *   or synchronised, and no argument changes from step to step, so the launch can be part of a captured graph. */
typedef struct jm_compose_desc
{
    int32_t n_sources;
    const int32_t * source_kind;        /* [n_sources] */
    const int32_t * source_rows;        /* [n_sources] */
    int32_t n_nodes;
    const int32_t * node_kind;          /* [n_nodes] */
    const int32_t * node_terminal;      /* [n_nodes] */
    const int32_t * node_normalized;    /* [n_nodes] */
    const int32_t * node_slot;          /* [n_nodes] */
    const int32_t * node_row;           /* [n_nodes] */
    const int32_t * node_child_start;   /* [n_nodes] */
    const int32_t * node_child_count;   /* [n_nodes] */
    const double * node_order;          /* [n_nodes] */
    int32_t n_children;
    const int32_t * child;              /* [n_children] */
    const double * child_weight;        /* [n_children] */
    int32_t n_conditions;
    const int32_t * cond_elem_start;    /* [n_conditions] */
    const int32_t * cond_elem_count;    /* [n_conditions] */
    const int32_t * cond_flags;         /* [n_conditions] */
    const double * cond_grace;          /* [n_conditions] */
    int32_t n_elements;
    const int32_t * elem_slot;          /* [n_elements] */
    const int32_t * elem_row;           /* [n_elements] */
    const int32_t * elem_bounds;        /* [n_elements] */
    const double * elem_low;            /* [n_elements] */
    const double * elem_high;           /* [n_elements] */
} jm_compose_desc;
typedef struct jm_compose_io
{
    const void * source[16];
    const void * time;
    const uint8_t * base_terminated;
    const uint8_t * base_truncated;
    const uint8_t * lane_mask;
    void * reward;
    void * node_value;
    uint8_t * terminated;
    uint8_t * truncated;
    int32_t * trigger;
    int32_t * violations;
} jm_compose_io;
typedef struct jm_compose_plan jm_compose_plan;
int32_t jm_compose_plan_create(const jm_compose_desc * desc, jm_compose_plan ** out);
int32_t jm_compose_plan_destroy(jm_compose_plan * plan);
int32_t jm_block_compose(const jm_compose_plan * plan, int32_t dtype, int64_t batch_size, const jm_compose_io * io, int32_t training,
                         void * stream);

/* ---- Observation assembly: `FlattenObservation(StackObservation(NormalizeObservation(ScaleObservation(
 * AdaptLayoutObservation(env)))))` as one launch, from the rows other blocks left on the device to the `(B, W)` tensor the learner
 * reads; batched, one lane = one environment, independent of the topology.  New symbols only: no existing structure or signature
 * changed with them.  Reference (python/gym_jiminy/common/gym_jiminy/common/wrappers): observation_layout.py:36-311, :314-443,
 * :446-540 (`_adapt_layout`, `AdaptLayoutObservation`, `FilterObservation`), scale.py:31-84, :141-244 (`_array_scale`,
 * `ScaleObservation`), normalize.py:49-114 (`NormalizeObservation`), observation_stack.py:40-265 (`StackObservation`), flatten.py
 * (`FlattenObservation`).
 * jm_observe_desc: the plan (host arrays, copied by jm_observe_plan_create, which validates them: JM_EINVAL + jm_last_error before
 *   any device call).
 *   Sources, 1 to 16: slot s is the base pointer `source[s]` of the launch, an array `[source_rows[s]][B]` of the input type.
 *   Elements, 1 to 2048 (D): one scalar of one kept leaf.  Element e reads (`elem_slot`, `elem_row`), is multiplied by the
 *     `elem_mult_count[e]` (at most 4) factors `multiplier[elem_mult_start[e] ..]` one after the other, each product rounded,
 *     and becomes `(x - elem_mean[e]) / elem_scale[e]` (0 and 1 where the leaf is not normalised; a zero scale is refused).
 *   `num_stack`, 1 to 16.  Positions, 1 to 8192 (W): column p of the output holds element `pos_elem[p]` at age `pos_age[p]`
 *     (0: the current frame).  An element is emitted once at age 0 (not stacked) or once at every age (stacked).
 * jm_observe_io: the device pointers of one launch.  `source[16]`; `reset_mask` (uint8 `[B]`, NULL: none): lanes whose older
 *   frames restart from zero; `hist` `[num_stack][D][B]` of the input type, owned by the caller, zero at creation (the rows of
 *   an element that is not stacked are never touched); `out` `[B][W]` of the output type, which may alias neither a source nor
 *   the history (JM_EINVAL).
 * jm_block_observe: `shift` != 0 moves every frame one age up before the current frame is written (`skip_frames_ratio` of the
 *   reference skips that on some steps: the current frame is then overwritten in place).  (dtype_in, dtype_out) is float64 ->
 *   float64, float64 -> float32 or float32 -> float32; the cast is the last operation.  Nothing is allocated, copied or
 *   synchronised. */
typedef struct jm_observe_desc
{
    int32_t n_sources;
    const int32_t * source_rows;        /* [n_sources] */
    int32_t n_elements;
    const int32_t * elem_slot;          /* [n_elements] */
    const int32_t * elem_row;           /* [n_elements] */
    const int32_t * elem_mult_start;    /* [n_elements] */
    const int32_t * elem_mult_count;    /* [n_elements] */
    const double * elem_mean;           /* [n_elements] */
    const double * elem_scale;          /* [n_elements] */
    int32_t n_multipliers;
    const double * multiplier;          /* [n_multipliers] */
    int32_t num_stack;
    int32_t n_positions;
    const int32_t * pos_elem;           /* [n_positions] */
    const int32_t * pos_age;            /* [n_positions] */
} jm_observe_desc;
typedef struct jm_observe_io
{
    const void * source[16];
    const uint8_t * reset_mask;
    void * hist;
    void * out;
} jm_observe_io;
typedef struct jm_observe_plan jm_observe_plan;
int32_t jm_observe_plan_create(const jm_observe_desc * desc, jm_observe_plan ** out);
int32_t jm_observe_plan_destroy(jm_observe_plan * plan);
int32_t jm_block_observe(const jm_observe_plan * plan, int32_t dtype_in, int32_t dtype_out, int64_t batch_size, const jm_observe_io * io,
                         int32_t shift, void * stream);

/* Copy the message of the last error raised on the calling thread. */
int32_t jm_last_error(char * buffer, size_t size);

#ifdef __cplusplus
}
#endif
#endif /* JIMINY_HIP_H */
