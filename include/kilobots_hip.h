/*
 * kilobots_hip.h -- C ABI of libkilobots_hip.so: the MI355X (gfx950) batched Kilobot world step.
 *
 * This is the drop-in boundary for the one hot path this library replaces: the substep loop of
 * gym-kilobots' `KilobotsEnv.step` (reference gym_kilobots/envs/kilobots_env.py:161-215), i.e.
 * light step -> light sensing -> per-kilobot drive law -> Box2D `world.Step(0.1, 10, 10)` ->
 * pose read-back, executed for num_envs x num_bots agents per launch.
 *
 * The reference has no FFI of its own (it is Python calling the SWIG module `Box2D`); every
 * entry point below cites the reference Python interface it replaces.  The Python binding
 * (ctypes) is gym_kilobots_amd/_native.py; INTEGRATION.md shows the stub a maintainer of the
 * reference would add.
 *
 * Conventions
 *   - every function returns 0 on success, a negative KB_E* code otherwise;
 *     kb_last_error() returns a thread-local message for the last failure;
 *   - nothing throws across the ABI;
 *   - all `d_*` pointers are DEVICE pointers owned by the caller (e.g. torch tensors); the
 *     library allocates no device memory.  Buffers bound with kb_bind() must stay alive until
 *     kb_destroy() or the next kb_bind();
 *   - all work is enqueued asynchronously on the `hipStream_t` passed as `void *stream`
 *     (NULL = the null stream); no call synchronises the device;
 *   - a handle is not thread-safe; distinct handles are independent;
 *   - arrays are SoA, shape [num_envs][num_bots], env-major, float32 unless noted;
 *   - body poses are Box2D world units = metres x 25 (reference gym_kilobots/lib/body.py:7),
 *     exactly what the reference's b2Body holds; kb_get_poses() converts to metres like
 *     Body.get_pose (body.py:63-65).
 */
#ifndef KILOBOTS_HIP_H
#define KILOBOTS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KB_OK 0
#define KB_EINVAL (-1)      /* bad argument / unsupported configuration */
#define KB_ENOTBOUND (-2)   /* kb_bind() has not been called or a required buffer is NULL */
#define KB_EHIP (-3)        /* a HIP runtime call failed */
#define KB_ELDS (-4)        /* configuration does not fit the 160 KiB LDS of a CU */

/* drive laws: which reference Kilobot subclass every bot of the handle is */
enum kb_drive_mode {
    KB_DRIVE_VELOCITY = 0,          /* SimpleVelocityControlKilobot      kilobot.py:213-263 */
    KB_DRIVE_ACCEL = 1,             /* SimpleAccelerationControlKilobot  kilobot.py:266-300 */
    KB_DRIVE_MOTORS = 2,            /* Kilobot.step motor law            kilobot.py:86-127  */
    KB_DRIVE_SIMPLE_PHOTOTAXIS = 3, /* SimplePhototaxisKilobot           kilobot.py:171-210 */
    KB_DRIVE_PHOTOTAXIS = 4,        /* PhototaxisKilobot                 kilobot.py:303-333 */
    KB_DRIVE_MIXED = 5              /* any mix of the five in one env (KilobotsEnv.step steps whatever is in _kilobots,
                                       kilobots_env.py:183-184): the law of every kilobot comes from kb_buffers.bot_mode, the
                                       fixture density of its class from kb_config.mode_density; every per-law state buffer is
                                       required; spill-free 256-VGPR instantiations: one-wave workgroups up to 128 kilobots,
                                       the full workgroup (one env per CU) beyond */
};

enum kb_light_type {
    KB_LIGHT_NONE = 0,
    KB_LIGHT_CIRCULAR = 1,          /* CircularGradientLight             light.py:151-195   */
    KB_LIGHT_GRADIENT = 2,          /* GradientLight                     light.py:218-271   */
    KB_LIGHT_MOMENTUM = 3,          /* MomentumLight                     light.py:274-319   */
    KB_LIGHT_COMPOSITE = 4          /* CompositeLight of <= 4 circular / momentum lights, light.py:99-148 */
};
#define KB_MAX_LIGHTS 4

/* kb_step flags */
#define KB_STEP_NO_DRIVE 1          /* world.Step only, kilobot body velocities = 0:
                                       KilobotsEnv._step_world, kilobots_env.py:217-219 */

#define KB_MAX_OBJECTS 8
#define KB_MAX_POLY_VERTS 4
/* fixture of a pushable object (body.py): Circle :181-192, Quad / CornerQuad :129-178 (b2PolygonShape::SetAsBox),
 * single-fixture convex Polygon :217-262 (b2PolygonShape::Set) */
enum kb_shape { KB_SHAPE_CIRCLE = 0, KB_SHAPE_BOX = 1, KB_SHAPE_POLYGON = 2 };
#define KB_OWS_COLS 12      /* object warm-start table: column = partner object 0..7, or 8 + wall */
#define KB_OWS_WORDS 6      /* per entry: (feature id, normal impulse, tangent impulse) of <= 2 manifold points; id < 0 = none */
#define KB_MAX_BOTS 1024

/* Scene constants.  Defaults of the reference are given in brackets. */
typedef struct kb_config {
    int32_t num_envs, num_bots, num_objects;    /* num_objects: 0..8 pushable bodies per env (the same shapes in every env) */
    float world_width, world_height;            /* metres [2.0, 1.5]   kilobots_env.py:19 */
    float dt;                                   /* [0.1]               kilobots_env.py:25,32 */
    int32_t vel_iters, pos_iters;               /* [10, 10]            kilobots_env.py:26-27 */
    int32_t drive_mode, light_type;
    float bot_radius;                           /* metres [0.0165]     kilobot.py:9 */
    float bot_density;                          /* [1.0; 2.0 for the velocity/accel bots] kilobot.py:25,214 */
    float bot_linear_damping, bot_angular_damping; /* [0.8, 0.8]       kilobot.py:29-30 */
    float light_radius;                         /* metres [0.2]        light.py:152 */
    float light_lo[2], light_hi[2];             /* light position bounds, light.py:44-46 */
    float light_act_lo[2], light_act_hi[2];     /* [-0.01, 0.01]       light.py:49-54 */
    float light_max_velocity;                   /* MomentumLight.max_velocity, light.py:289-292 */
    int32_t ws_slots;                           /* warm-start slots per bot [8] */
    float obj_radius[KB_MAX_OBJECTS];           /* metres; Circle(radius=...), body.py:181-192 */
    float obj_density, obj_friction;            /* [2, 0.01] body.py:11-12 */
    float obj_linear_damping, obj_angular_damping; /* [0.8, 0.8] body.py:15-16 */
    int32_t toi_walls;                          /* [1] b2World::SolveTOI against the static walls (continuousPhysics) */
    int32_t solver_mode;                        /* 0 = automatic.  Test knobs (results are identical in every mode):
                                                   1 list solver, one wave per island set; 2 list solver, whole
                                                   workgroup per sweep; 3 / 4 = 1 / 2 with contacts staged in `scratch` */
    /* KB_LIGHT_COMPOSITE only: the component lights (the fields above then are unused) */
    int32_t light_count;                        /* 1..KB_MAX_LIGHTS */
    int32_t light_kind[KB_MAX_LIGHTS];          /* KB_LIGHT_CIRCULAR or KB_LIGHT_MOMENTUM */
    float lightc_radius[KB_MAX_LIGHTS], lightc_max_velocity[KB_MAX_LIGHTS];
    float lightc_lo[KB_MAX_LIGHTS][2], lightc_hi[KB_MAX_LIGHTS][2];
    float lightc_act_lo[KB_MAX_LIGHTS][2], lightc_act_hi[KB_MAX_LIGHTS][2];
    /* objects other than circles */
    int32_t obj_shape[KB_MAX_OBJECTS];          /* enum kb_shape [circle] */
    int32_t obj_nverts[KB_MAX_OBJECTS];         /* KB_SHAPE_POLYGON: 3..KB_MAX_POLY_VERTS */
    float obj_verts[KB_MAX_OBJECTS][KB_MAX_POLY_VERTS][2]; /* body frame, Box2D WORLD UNITS: metres x 25 evaluated in double and
                                                   then rounded, exactly what body.py:137,246 hands to Box2D.
                                                   BOX: [0] = (width / 2, height / 2) x 25 (Quad, body.py:136-137).
                                                   POLYGON: counter-clockwise hull in b2PolygonShape::Set order, centred on
                                                   its centroid (body.py:226-241) */
    float wall_friction;                        /* [0.2] b2FixtureDef default of the arena chain, kilobots_env.py:46-51 */
    /* bodies with several convex fixtures (LForm, TForm, CForm: body.py:277-334).  With num_fixtures > 0 the arrays
     * obj_shape / obj_nverts / obj_verts / obj_radius are indexed by FIXTURE and fixture f belongs to object
     * obj_fixture_body[f] (fixtures of one object need not be adjacent); num_fixtures == 0 means one fixture per
     * object.  Mass, centre of mass and inertia follow b2Body::ResetMassData; ox / oy hold the body ORIGIN like
     * Body.get_pose (body.py:63-65), ovx / ovy the velocity of the centre of mass like b2Body::GetLinearVelocity. */
    int32_t num_fixtures;                       /* 0, or num_objects..KB_MAX_OBJECTS (at most 8 fixtures per env in total) */
    int32_t obj_fixture_body[KB_MAX_OBJECTS];
    int32_t damping_model;                      /* [KB_DAMPING_PADE] how b2Island::Solve applies linearDamping / angularDamping
                                                   (body.py:15-16,35-36): Box2D >= 2.3.1 `v *= 1 / (1 + h c)`, Box2D <= 2.3.0
                                                   `v *= clamp(1 - h c, 0, 1)`.  The reference does not pin box2d-py (setup.py:5);
                                                   INTEGRATION.md says how to tell which one an installed wheel uses. */
    float sense_radius;                         /* metres, centre to centre; 0 = off.  IR-range neighbour sensing (no counterpart in
                                                   the reference; nearest: Body.collides_with, body.py:87-90): at the sensing point
                                                   of every substep (kilobots_env.py:174-180, before the drive law) kilobot i counts
                                                   the kilobots j != i of its env with |p_j - p_i|^2 <= (25 R)^2 in fp32 world units;
                                                   kb_buffers.nbr_count holds the counts of the last substep */
    int32_t contact_capacity;                   /* [0] contacts (and warm-start entries) per env; 0 = the default rule
                                                   max(4 N + 64, min(N (N - 1) / 2 + 4 N, 2304)) + 40 objects.  A spawn that
                                                   overlaps more kilobots than that sets status bit 0; raise it (<= 65528) then:
                                                   the entries live in HBM (36 B each), not in LDS */
    float mode_density[5];                      /* KB_DRIVE_MIXED: fixture density of the kilobots of drive law k (Kilobot._density 1.0,
                                                   SimpleVelocityControlKilobot._density 2.0: kilobot.py:25, :214); 0 = bot_density */
    int32_t allow_sleep;                        /* [1 in the helpers that fill a default config; 0 leaves the state out] b2World(gravity, doSleep=True) of kilobots_env.py:45: bodies carry
                                                   b2Body::m_sleepTime (kb_buffers.sleep_time / osleep, seconds; < 0: asleep).  An
                                                   island whose bodies all stayed below b2_linearSleepTolerance /
                                                   b2_angularSleepTolerance for b2_timeToSleep = 0.5 s and whose position
                                                   constraints converged falls asleep (b2Island::Solve: velocities zeroed); islands
                                                   without an awake body are not simulated (b2World::Solve); a body wakes when a
                                                   non-zero velocity is assigned to it (Kilobot.step -> b2Body::SetLinearVelocity /
                                                   SetAngularVelocity) or an awake island reaches it.  The envs of
                                                   gym_kilobots_amd.envs switch it on like the reference; bench.py's headline
                                                   runs without the state (sleeping cannot change a trajectory in which every
                                                   kilobot is commanded to move in every substep: DESIGN.md 4c) and reports the
                                                   instantiation with it next to it */
} kb_config;

enum kb_damping_model { KB_DAMPING_PADE = 0, KB_DAMPING_LINEAR = 1 };

/* Device buffers of one handle.  NULL is allowed for buffers the configuration never touches
 * (noted per field).  Replaces the per-object state of the reference: b2Body position/angle
 * (body.py:51-72), Kilobot._velocity / _acceleration / _motor_* (kilobot.py:37-38,225-229,277),
 * PhototaxisKilobot counters (kilobot.py:307-313), light position (light.py:40-42). */
typedef struct kb_buffers {
    float *x, *y, *theta;               /* required */
    float *v, *w;                       /* VELOCITY / ACCEL modes: commanded (v [m/s], omega [rad/s]) */
    float *acc_v, *acc_w;               /* ACCEL mode */
    uint8_t *motor_l, *motor_r;         /* MOTORS / PHOTOTAXIS modes */
    float *pt_threshold;                /* PHOTOTAXIS mode */
    int32_t *pt_update, *pt_nochange;   /* PHOTOTAXIS mode */
    uint8_t *pt_dir;                    /* PHOTOTAXIS mode: 0 = 'left', 1 = 'right' */
    float *light_x, *light_y;           /* [num_envs][kb_light_count()], metres; GradientLight: its angle in light_x */
    float *light_vx, *light_vy;         /* [num_envs][kb_light_count()] MomentumLight velocity (light.py:284-287) */
    float *ox, *oy, *otheta, *ovx, *ovy, *ow; /* objects: [num_envs][num_objects] pose (world units, radians) and body velocity */
    /* warm-start store (Box2D keeps the accumulated normal impulse in each b2Contact): per env a packed
     * list of kb_contact_capacity() entries, owner bots ascending, ws_cnt[bot] entries per owner.  The tail of the list, the
     * positions from min(sum of ws_cnt[env], kb_contact_capacity()) on, means nothing: no entry point ever reads it, and
     * whatever it holds changes no result */
    uint32_t *ws_key;                   /* required: [num_envs][kb_contact_capacity()] */
    float *ws_acc;                      /* required: [num_envs][kb_contact_capacity()] */
    uint8_t *ws_cnt;                    /* required: [num_envs][num_bots]; zero it to forget all contacts */
    float *light_value, *light_gx, *light_gy; /* optional outputs: last sensed light (kilobots_env.py:176-180) */
    float *cmd_vx, *cmd_vy, *cmd_w;     /* optional outputs: body velocity written by the drive law */
    int32_t *status;                    /* required: [num_envs]; bit0 contact capacity overflow,
                                           bit1 warm-start slot overflow, bit2 a device staging limit was exceeded in one substep of
                                           the env (the env is then flagged, not bit-exact; each number is the largest that is
                                           still exact): 255 as the largest rank in one group of contacts -- 256 kilobot-kilobot
                                           contacts whose owners lie in one cell and whose partners lie in one of the five
                                           directions same cell, E, N, NE, NW of it; 63 partners of one kilobot in one such
                                           direction (never the first to be exceeded: 63 kilobots in one cell within reach of one
                                           kilobot touch each other in more than 256 pairs); 64 kilobots on one fixture (kernels
                                           with objects or mixed drive laws); and -- kernels without objects, an env swept level by
                                           level by a workgroup of two waves or more -- 44 x waves of the workgroup - 2 levels of
                                           contacts that depend on each other (86 at two waves; a one-wave workgroup sweeps its
                                           lists and has no such limit),
                                           bit3 more kilobots that may meet a wall in the continuous step of one substep than the
                                           kernel keeps candidates for (the continuous step is skipped for the rest); the largest
                                           number it keeps: min(kb_lds_staging_entries(), num_bots) in the kernels without objects
                                           (688 at 1024 kilobots; a staging area of num_bots entries or more cannot run out; a small
                                           contact_capacity shrinks the staging area with it), kb_lds_staging_entries() / 2 in the
                                           kernels with objects or mixed drive laws.  tests/limits_model.py restates every one of
                                           these counts on the CPU */
    void *scratch;                      /* required: kb_scratch_bytes() bytes; contact staging of envs whose
                                           contacts do not fit the LDS staging area (contents are transient: no launch
                                           reads a byte of it that the same launch has not written before, so it
                                           carries nothing from launch to launch and may hold anything) */
    float *ows_acc;                     /* objects: [num_envs][8][KB_OWS_COLS][KB_OWS_WORDS] manifold impulses of the
                                           object-object (column = higher partner) and object-wall (column 8 + wall)
                                           contacts: b2ManifoldPoint id / normalImpulse / tangentImpulse; fill with -1
                                           to forget them */
    uint32_t *nbr_count;                /* sense_radius > 0: [num_envs][num_bots] neighbours within IR range (output; required then) */
    float *sleep_time;                  /* allow_sleep: [num_envs][num_bots] b2Body::m_sleepTime in seconds, < 0 = asleep (required then;
                                           zero-fill = awake) */
    float *osleep;                      /* allow_sleep with objects: the same for the objects, [num_envs][num_objects] */
    uint8_t *bot_mode;                  /* KB_DRIVE_MIXED: [num_envs][num_bots] drive law of every kilobot (KB_DRIVE_VELOCITY ..
                                           KB_DRIVE_PHOTOTAXIS; required then) */
} kb_buffers;

typedef struct kb_sim kb_sim;

/* Replaces KilobotsEnv.__init__ world construction (kilobots_env.py:45-51: b2World + chain-loop
 * walls) and Body/Circle/Kilobot fixture constants (body.py:32-38,187-192; kilobot.py:9-30). */
int kb_create(const kb_config *cfg, kb_sim **out);
void kb_destroy(kb_sim *sim);

/* Attach caller-owned device buffers (copied by value). */
int kb_bind(kb_sim *sim, const kb_buffers *buf);

/* SimpleVelocityControlKilobot.set_action / SimpleAccelerationControlKilobot.set_action
 * (kilobot.py:235-241, 283-289), as called per bot by DirectControlKilobotsEnv.step
 * (direct_control_kilobots_env.py:18-27).  d_actions: [num_envs][num_bots][2] or NULL (= None). */
int kb_set_actions(kb_sim *sim, const float *d_actions, void *stream);

/* n_substeps iterations of the KilobotsEnv.step loop body (kilobots_env.py:168-190) in ONE launch.
 * d_actions (optional): kilobot actions applied first, as kb_set_actions.
 * d_light_action (optional): [num_envs][kb_light_action_dim()] light action (2 per positional light in
 * component order, 1 for a GradientLight), applied every substep (kilobots_env.py:171-172);
 * NULL = action None. */
int kb_step(kb_sim *sim, const float *d_actions, const float *d_light_action, int n_substeps, int flags,
            void *stream);

/* kb_step for the envs a mask selects; the others stay frozen (evaluation with finished envs, the resolve step of
 * kb_reset_envs).  d_env_mask: [num_envs] bytes in device memory, non-zero = selected (a bool tensor as it stands).
 *   - A selected env is stepped exactly as kb_step steps it, the fused d_actions included.
 *   - For an unselected env NO BYTE of any bound buffer changes: poses, commands (the fused set_action does not reach it), the
 *     warm-start store, sleep_time, nbr_count, status, the light state, the debug outputs.  kb_buffers.scratch is transient by
 *     contract and excluded.
 *   - The mask is read once, at the start of the launch, also when n_substeps > 1: the workgroup of an unselected env leaves
 *     before it has read or written anything else.
 *   - One launch of the handle's own instantiation on the same grid; kb_step is this call without a mask.
 * Argument checks in this order: NULL sim or NULL mask -> KB_EINVAL;  an unbound handle -> KB_ENOTBOUND;  then those of
 * kb_step.  Asynchronous on `stream`. */
int kb_step_envs(kb_sim *sim, const uint8_t *d_env_mask, const float *d_actions, const float *d_light_action, int n_substeps,
                 int flags, void *stream);

/* IR-range neighbour sensing on the CURRENT poses, without stepping (e.g. right after a reset): d_count
 * [num_envs][num_bots] uint32 = number of kilobots j != i of the same env with |p_j - p_i|^2 <= (25 radius_m)^2.
 * The same predicate kb_step evaluates at the sensing point of every substep when kb_config.sense_radius > 0.
 * No reference counterpart (the reference has no neighbour sensing; nearest: Body.collides_with, body.py:87-90). */
int kb_sense(kb_sim *sim, float radius_m, uint32_t *d_count, void *stream);

/* Nearest-neighbour lists on the CURRENT poses, without stepping: for every kilobot i the k nearest kilobots j != i of
 * the same env within IR range, with their offsets in the body frame of i -- what a decentralised policy observes.
 * No reference counterpart.  Every operation below is one fp32 operation rounded on its own:
 *   Rw = radius_m * 25, R2 = Rw * Rw (on the host, as kb_sense);  ex = x_j - x_i, ey = y_j - y_i (world units);
 *   d2 = ex * ex + ey * ey;  j is in range iff !(d2 > R2) (the predicate of kb_sense);
 *   neighbours are ordered by (d2, j) ascending, ties go to the lower index; the first min(k, count) are written;
 *   (s, c) = the library's sine and cosine of theta_i (the Cephes algorithm every kernel uses);
 *   rel[0] = (c * ex + s * ey) / 25   metres ahead         rel[1] = (c * ey - s * ex) / 25   metres to the left
 *   rel[2] = sqrt(d2) / 25            distance in metres   rel[3] = theta_j - theta_i        (not wrapped)
 *   with correctly rounded divisions and square root.
 * d_index [num_envs][num_bots][k] int32: index of the neighbour within its env, -1 in unused slots.
 * d_rel   [num_envs][num_bots][k][4] float32, 16-byte aligned: rel of each slot, all 0.0f in unused slots.
 * d_count [num_envs][num_bots] uint32 or NULL: kilobots in range (may exceed k) -- what kb_sense writes for this radius.
 * 1 <= k <= KB_MAX_NEIGHBORS.  Reads x, y, theta; writes the three outputs only.  Asynchronous on `stream`. */
#define KB_MAX_NEIGHBORS 16
int kb_sense_neighbors(kb_sim *sim, float radius_m, int k, int32_t *d_index, float *d_rel, uint32_t *d_count,
                       void *stream);

/* The whole IR-range graph on the CURRENT poses, without stepping: every pair of kilobots of an env in IR range, as a CSR /
 * COO edge list over the whole batch -- the ragged output that graph networks, learned message passing and connectivity
 * metrics consume, and that the fixed-size rows of kb_sense_neighbors truncate at 16.  No reference counterpart.  Every
 * operation is one fp32 operation rounded on its own.
 *   Nodes: node ids are local to the handle; kilobot i of env e is node r = e * num_bots + i.  num_envs * num_bots < 2^31
 *     (KB_EINVAL otherwise).
 *   Predicate: as kb_sense -- Rw = radius_m * 25, R2 = Rw * Rw (on the host);  ex = x_j - x_i, ey = y_j - y_i,
 *     d2 = ex * ex + ey * ey;  j is a neighbour of i iff j != i && !(d2 > R2).
 *   Row of i: its neighbours in ASCENDING j; nothing else decides the order.  Both directions of a pair are present, (i, j)
 *     in the row of i and (j, i) in the row of j, each with the attributes of its own frame.
 *   rel[4] of an edge: as kb_sense_neighbors.
 * d_offsets [num_envs * num_bots + 1] int64: the CSR row pointer, supplied by the caller -- the exclusive prefix sum of the
 *   counts kb_sense gives at the same radius on the same poses (the library allocates nothing and does not scan).
 * d_dst   [capacity] int32: node id of j.
 * d_src   [capacity] int32 or NULL: node id of i.
 * d_rel   [capacity][4] float32, 16-byte aligned, or NULL.
 * d_count [num_envs][num_bots] uint32 or NULL: the true number of neighbours of every kilobot, whatever d_offsets says --
 *   what kb_sense writes for this radius.
 * Memory contract (d_offsets may be stale; it cannot make the call write out of bounds): row r owns the slots [lo, hi) with
 *   lo = d_offsets[r], hi = d_offsets[r + 1], both clipped to [0, capacity]; the row is empty if hi <= lo.  The first
 *   min(count_r, hi - lo) neighbours in ascending j are written there; the slots of the row beyond count_r receive dst = src
 *   = -1 and rel = +0.0 x 4.  Nothing is stored outside [0, capacity) and nothing in a slot that no row owns.  With consistent
 *   offsets every slot in [0, d_offsets[num_envs * num_bots]) is written exactly once, by plain stores.  (Offsets that do
 *   not ascend may make rows overlap; such a slot receives the value of one of its rows.)
 * Argument errors are reported before an unbound handle, in this order: NULL sim / d_offsets;  radius_m not > 0;
 * capacity < 0;  capacity > 0 with NULL d_dst.  Then KB_ENOTBOUND;  then a d_rel that is not 16-byte aligned;  then the node
 * count.  capacity == 0 is legal: with d_count it is the counting call; without it nothing is launched and the call returns
 * KB_OK -- after the checks above, so on an unbound handle it answers KB_ENOTBOUND like every other valid call.
 * Reads x, y, theta and d_offsets; writes the outputs only.  The result of an env does not depend on the other envs, apart
 * from where its rows start.  One launch.  Asynchronous on `stream`. */
int kb_sense_edges(kb_sim *sim, float radius_m, const int64_t *d_offsets, int64_t capacity, int32_t *d_src, int32_t *d_dst,
                   float *d_rel, uint32_t *d_count, void *stream);

/* Local neighbour histograms on the CURRENT poses, without stepping: for every kilobot i the number of kilobots j != i of
 * the same env within IR range, binned by distance (n_rings rings of equal width) and by bearing in the body frame of i
 * (n_sectors sectors of equal angle) -- a fixed-size, permutation-invariant observation that counts ALL neighbours in
 * range, however many there are.  No reference counterpart.  Every operation below is one fp32 operation rounded on its own:
 *   Rw = radius_m * 25, R2 = Rw * Rw (on the host, as kb_sense);  ex = x_j - x_i, ey = y_j - y_i (world units);
 *   d2 = ex * ex + ey * ey;  j is counted iff !(d2 > R2) (the predicate of kb_sense);
 *   ring: on the host, for r = 1 .. n_rings - 1, edge_r = (Rw * (float)r) / (float)n_rings and E2_r = edge_r * edge_r;
 *     ring = the number of r with d2 > E2_r (a neighbour exactly on an edge belongs to the inner ring);
 *   sector: (s, c) = the library's sine and cosine of theta_i (the Cephes algorithm every kernel uses);
 *     a = c * ex + s * ey (ahead), l = c * ey - s * ex (to the left), world units, NOT divided by 25;
 *     n_sectors == 1: sector = 0.  Otherwise H = n_sectors / 2, low = (l < 0), (a', l') = low ? (-a, -l) : (a, l),
 *     q = the number of m in 1 .. H - 1 with u_m.x * l' - u_m.y * a' > 0 (two products, one difference),
 *     sector = (low ? H : 0) + q: sector 0 starts dead ahead, the sectors run counter-clockwise.  A neighbour exactly on
 *     a boundary, one with l == +-0 and a coincident one (a = l = 0: sector 0) are decided by these comparisons alone;
 *   u_m = ((float)cos(pi m / H), (float)sin(pi m / H)) evaluated in double on the host and rounded to fp32, the entry
 *     with 2 m == H exactly (0, 1).  kb_histogram_sectors writes this very table, the one the kernel is handed, for
 *     m = 1 .. H - 1 into xy (HOST memory, [n_sectors / 2 - 1][2]); it needs no handle and no device, and returns
 *     KB_EINVAL for an illegal n_sectors or a NULL xy when the table is not empty.
 * d_hist  [num_envs][num_bots][n_rings][n_sectors] float32: neighbours in each bin (at most 1023: exact; float because it
 *         is a network input as it stands).  Every element is written by every call, the zeros included.
 * d_count [num_envs][num_bots] uint32 or NULL: kilobots in range = the sum of the row -- what kb_sense writes for this radius.
 * 1 <= n_rings <= KB_HIST_MAX_RINGS; n_sectors 1 or even in 2..KB_HIST_MAX_SECTORS; n_rings * n_sectors <= KB_HIST_MAX_BINS;
 * radius_m > 0 (a radius beyond the arena is fine).  Argument errors are reported before an unbound handle.
 * Reads x, y, theta; writes the two outputs only.  Asynchronous on `stream`. */
#define KB_HIST_MAX_RINGS 8
#define KB_HIST_MAX_SECTORS 16
#define KB_HIST_MAX_BINS 64
int kb_sense_histogram(kb_sim *sim, float radius_m, int n_rings, int n_sectors, float *d_hist, uint32_t *d_count,
                       void *stream);
int kb_histogram_sectors(int n_sectors, float *xy /* host, [n_sectors / 2 - 1][2] */);

/* IR-range message aggregation on the CURRENT poses, without stepping: every kilobot broadcasts a message of n_channels
 * floats, and every kilobot i combines, channel by channel, the messages of the kilobots j != i of the same env within IR
 * range -- the reduction behind gradient (hop-count) formation (min + 1), consensus (mean), leader election (max) and the
 * sum of a message-passing layer.  ALL kilobots in range take part, however many there are.  No reference counterpart.
 * Every reduction is independent of the order in which the neighbours are met: no two floats are ever added, so the
 * result is the same bit for bit in a shard.  Every operation below is one fp32 operation rounded on its own:
 *   Rw = radius_m * 25, R2 = Rw * Rw (on the host, as kb_sense);  ex = x_j - x_i, ey = y_j - y_i (world units);
 *   d2 = ex * ex + ey * ey;  j is heard by i iff !(d2 > R2) (the predicate of kb_sense);
 *   KB_REDUCE_SUM, a fixed-point sum: per broadcast value v, t = v * scale;  q = 0 if t is NaN, otherwise
 *     q = (int32) rint(clamp(t, -2^21, 2^21)), round half to even (+-inf become +-2^21);  acc = the sum of q_j over the
 *     kilobots heard, in int32 (1023 * 2^21 < 2^31: no overflow);  out = (float)acc / scale: int -> float to nearest even,
 *     then one correctly rounded division.  scale must be finite and > 0; with a power of two the quantisation is the only
 *     rounding.  The sum is exact on the quantised values; the mean is out / count, taken by the caller;
 *   KB_REDUCE_MIN / KB_REDUCE_MAX, in the total order of the bit patterns: key = bits ^ (bits >> 31 ? 0xFFFFFFFF :
 *     0x80000000) compared unsigned, so -0 < +0, NaNs with the sign bit clear sort above +inf and those with it set below
 *     -inf;  out = the value heard whose key is smallest / largest, bit pattern preserved.  scale is ignored;
 *   nothing heard: SUM gives +0.0, MIN +inf, MAX -inf (the identities: h = min(h, reduce_min(h) + 1) needs no special case).
 * d_values [num_envs][num_bots][n_channels] float32: what every kilobot broadcasts.
 * d_out    [num_envs][num_bots][n_channels] float32: what every kilobot has heard.  d_out == d_values (the same pointer)
 *          is allowed: every env is read whole before any of it is written.  Any other overlap is undefined.
 * d_count  [num_envs][num_bots] uint32 or NULL: kilobots heard -- what kb_sense writes for this radius.
 * 1 <= n_channels <= KB_REDUCE_MAX_CHANNELS; op is one of kb_reduce_op; radius_m > 0 (a radius beyond the arena is fine).
 * Argument errors (NULL sim / d_values / d_out, then op, n_channels, radius_m and, for KB_REDUCE_SUM, scale) are reported
 * before an unbound handle.  Reads x, y and d_values; writes d_out and d_count only, every element on every call.
 * Asynchronous on `stream`. */
enum kb_reduce_op { KB_REDUCE_SUM = 0, KB_REDUCE_MIN = 1, KB_REDUCE_MAX = 2 };
#define KB_REDUCE_MAX_CHANNELS 8
int kb_sense_reduce(kb_sim *sim, float radius_m, int op, int n_channels, float scale, const float *d_values, float *d_out,
                    uint32_t *d_count, void *stream);

/* Hop-count gradients on the CURRENT poses, without stepping: for every kilobot the number of IR hops to the nearest seed of
 * its env -- the quantity behind self-assembly, leader election, routing and the question whether the swarm is connected --
 * settled by one breadth-first search per env in ONE launch, instead of one kb_sense_reduce(min) sweep per hop.  Every env is
 * searched independently.  No reference counterpart.  All results are integers; the only float arithmetic is the predicate:
 *   Graph: as kb_sense -- Rw = radius_m * 25, R2 = Rw * Rw (on the host);  ex = x_j - x_i, ey = y_j - y_i,
 *     d2 = ex * ex + ey * ey (each one fp32 operation rounded on its own);  j is a neighbour of i iff j != i && !(d2 > R2).
 *     The relation is symmetric bit for bit.  Poses are assumed finite, as everywhere else.
 * d_seed   [num_envs][num_bots] uint8 in device memory: non-zero = seed (the convention of d_env_mask; a bool tensor works
 *          as it stands).
 * d_hops   [num_envs][num_bots] int32: 0 for a seed; for any other kilobot the least number of edges on a path to any seed
 *          of its env if that number is <= max_hops; otherwise -1 (unreachable, or cut by max_hops).
 * d_parent [num_envs][num_bots] int32 or NULL: -1 for seeds and for kilobots with hops -1; otherwise the LOWEST index j
 *          within the env that is a neighbour of i and has hops[j] == hops[i] - 1.  Nothing else decides it: not the order
 *          of the cell lists and not the order in which the search reaches i.
 * d_root   [num_envs][num_bots] int32 or NULL: a seed gets its own index, a reached kilobot root[parent[i]] -- the seed at
 *          the end of its parent chain, i.e. the graph-Voronoi assignment to the seeds with ties resolved by the parent
 *          rule; -1 where hops is -1.
 * d_stats  [num_envs][2] int32 or NULL: word 0 the number of kilobots with hops >= 0 (seeds included), word 1 the largest
 *          value in the env's hops, -1 when the env has no seed.  With one seed, stats[0] == num_bots says: connected.
 * max_hops >= 0: with 0 only the seeds are reached; any value >= num_bots - 1 cuts nothing, and KB_HOPS_UNLIMITED is the
 *          spelled-out way to ask for that.
 * Argument errors are reported before an unbound handle, in this order: NULL sim / d_seed / d_hops;  radius_m not > 0;
 * max_hops < 0.  Then KB_ENOTBOUND.  A radius beyond the arena is fine (the reach clamps to the grid).
 * Reads x, y and d_seed; writes only the outputs that were given, every element of each on every call, by plain stores.
 * The result of an env does not depend on the other envs: a shard reproduces its rows.  One launch.  Asynchronous on
 * `stream`. */
#define KB_HOPS_UNLIMITED KB_MAX_BOTS
int kb_sense_hops(kb_sim *sim, float radius_m, const uint8_t *d_seed, int max_hops, int32_t *d_hops, int32_t *d_parent,
                  int32_t *d_root, int32_t *d_stats, void *stream);

/* Connected components of the IR-range graph on the CURRENT poses, without stepping: which kilobots hang together, in how
 * many groups, and how large the largest one is -- "largest cluster / num_bots" is the aggregation metric of the swarm
 * literature -- settled by one union-find per env in ONE launch, where kb_sense_hops needs a seed per component and a sweep
 * over kb_sense_edges needs as many rounds as the graph's diameter.  Every env is labelled independently.  No reference
 * counterpart.  Labels, sizes and stats are integers; the float arithmetic is the predicate and the table:
 *   Nodes: the kilobots b of the env with d_select[e][b] != 0 (bytes, the convention of d_seed; a bool tensor works as it
 *     stands); NULL: all of them.  A kilobot that is not selected is not in the graph: it connects nothing.
 *   Edges: as kb_sense and kb_sense_hops -- Rw = radius_m * 25, R2 = Rw * Rw (on the host);  ex = x_j - x_i, ey = y_j - y_i,
 *     d2 = ex * ex + ey * ey (each one fp32 operation rounded on its own);  nodes i and j are joined iff j != i && !(d2 > R2).
 *     The relation is symmetric bit for bit.  Poses are assumed finite, as everywhere else.
 * d_label   [num_envs][num_bots] int32, required: for a node the LOWEST index of its connected component, -1 for a kilobot
 *           that is not selected.  Nothing else decides it: not the order of the cell lists and not the order in which the
 *           kernel joins the pairs.
 * d_size    [num_envs][num_bots] int32 or NULL: the number of nodes in the kilobot's component; 0 for one that is not selected.
 * d_cluster [num_envs][num_bots][4] float32, 16-byte aligned, or NULL: row r of env e describes the component whose label is r;
 *           every other row is four +0.0f.  A kilobot finds the row of its component at d_cluster[e][label].  With n the
 *           number of members:
 *     q = (int64) rint(max(min(v * 65536.0f, 0x1p40f), -0x1p40f)), round half to even, for each member coordinate v (x or y);
 *     SX, SY = the int64 sums of q over the members;
 *     cxw = ((float)SX / (float)n) / 65536.0f, cyw likewise (int64 -> float to nearest even, correctly rounded divisions);
 *     per member:  ex = x_b - cxw, ey = y_b - cyw, d2 = ex * ex + ey * ey;  D = the largest d2 of a member (the maximum of
 *     the bit patterns);
 *     the row is ((float)n, cxw / 25.0f, cyw / 25.0f, sqrt(D) / 25.0f): the size, the centroid in metres in the world frame, the
 *     distance of the farthest member from it in metres.  Exact on the quantised values and independent of any order.
 * d_stats   [num_envs][4] int32 or NULL: word 0 the number of components; word 1 the size of the largest, 0 without a node;
 *           word 2 the label of the largest, ties to the LOWEST label, -1 without a node; word 3 the number of components of
 *           size 1 (isolated kilobots).  stats[1] / num_bots is the aggregation metric; stats[0] == 1 says: connected.
 * Each optional output may be NULL and is then not computed; every element of every output given is written on every call, by
 * a plain store (nothing needs clearing beforehand).  The result of an env does not depend on the other envs: a shard
 * reproduces its rows.
 * Argument errors are reported before an unbound handle, in this order: NULL sim / d_label;  radius_m not > 0;  a d_cluster
 * that is not 16-byte aligned.  Then KB_ENOTBOUND.  A radius beyond the arena is fine (the reach clamps to the grid).
 * Reads x, y and d_select; writes the outputs only.  One launch.  Asynchronous on `stream`. */
int kb_sense_clusters(kb_sim *sim, float radius_m, const uint8_t *d_select, int32_t *d_label, int32_t *d_size, float *d_cluster,
                      int32_t *d_stats, void *stream);

/* Object and wall points on the CURRENT poses, without stepping: for every kilobot i and every pushable object m of its env
 * the nearest point of the object's outline in the body frame of i, and the nearest point of the arena walls -- what a
 * decentralised policy sees of the thing it pushes and of what confines it.  Rows are fixed-size, one per object, in object
 * order; there is no range cut.  No reference counterpart.  Every operation below is one fp32 operation rounded on its own,
 * with correctly rounded divisions and square roots; all lengths are world units until the final / 25:
 *   (si, ci) = the library's sine and cosine of theta_i (the Cephes algorithm every kernel uses).
 *   Per object m, (so, co) = sine and cosine of otheta_m:  dx = x_i - ox_m, dy = y_i - oy_m;  the kilobot in the object's
 *     frame is px = co * dx + so * dy, py = co * dy - so * dx.
 *   Candidates come from the fixtures of object m in the order of kb_get_outline:
 *     polygon (and box) fixture, edge k from a = v[k] to b = v[(k + 1) % n]:  ex = b.x - a.x, ey = b.y - a.y;
 *       wx = px - a.x, wy = py - a.y;  t = (wx * ex + wy * ey) / (ex * ex + ey * ey);
 *       q = a if !(t > 0) (NaN included), q = b if t >= 1, otherwise q = (a.x + t * ex, a.y + t * ey);
 *       rx = q.x - px, ry = q.y - py;  d2 = rx * rx + ry * ry;  cr = ex * wy - ey * wx: the centre is inside the fixture
 *       iff cr >= 0 on all of its edges;
 *     circle fixture of radius r (centred on the body origin):  n2 = px * px + py * py, n = sqrt(n2), g = n - r;
 *       n > 0: rx = -(g * (px / n)), ry = -(g * (py / n));  otherwise (rx, ry) = (r, 0);  d2 = g * g;  inside iff !(g > 0).
 *   The candidate with the smallest d2 wins (d2 < the best so far, starting from +inf with r = (0, 0)); ties go to the
 *     earlier candidate: the lower fixture in outline order, then the lower edge.
 *   gx = co * rx - so * ry, gy = so * rx + co * ry (world frame);
 *   obj = ((ci * gx + si * gy) / 25 metres ahead, (ci * gy - si * gx) / 25 metres to the left, sqrt(d2) / 25 distance in metres,
 *          1.0f if the centre is inside ANY fixture of the object, else 0.0f).
 *   With the centre inside, the point is the nearest fixture EDGE; on a body with several fixtures (LForm, TForm, CForm)
 *   that may be an interior edge, where two fixtures meet, and not a point of the body's outer outline.
 *   Walls: g0 = x_i - xmin, g1 = xmax - x_i, g2 = y_i - ymin, g3 = ymax - y_i; the smallest gap g wins, ties go to the lower
 *     index; a kilobot outside the arena has a negative gap, and that gap wins.  The world vector to the wall point is
 *     (-g0, 0), (g1, 0), (0, -g2) or (0, g3), rotated like (gx, gy):
 *   wall = (ahead / 25, left / 25, g / 25 (signed), (float)index).
 * d_obj  [num_envs][num_bots][num_objects][4] float32, 16-byte aligned, or NULL.
 * d_wall [num_envs][num_bots][4] float32, 16-byte aligned, or NULL.  Both NULL is KB_EINVAL, and so is a non-NULL d_obj on a
 * handle with num_objects == 0.  Argument errors are reported before an unbound handle.
 * Reads x, y, theta, ox, oy, otheta; writes the two outputs only, every element on every call.  Asynchronous on `stream`.
 *
 * kb_get_outline: the geometry kb_sense_objects reads, exactly as its kernel is handed it -- the fixture tables kb_create
 * derived and the arena bounds.  Fixtures are grouped by body in stable order (body 0's fixtures first; within a body they
 * keep their kb_config order): the order the kernel walks and the order that decides ties.  Host only: needs no device and
 * no bound buffers. */
typedef struct kb_outline {
    int32_t num_objects, num_fixtures;          /* num_fixtures: the fixtures of the handle (>= num_objects) */
    float arena[4];                             /* xmin, xmax, ymin, ymax in fp32 world units */
    int32_t body[KB_MAX_OBJECTS], kind[KB_MAX_OBJECTS], nverts[KB_MAX_OBJECTS];  /* per fixture, in the order the kernel visits
                                                   them: its object, enum kb_shape, vertices (circles: 0, boxes: 4) */
    float radius[KB_MAX_OBJECTS];               /* circles: world units; polygons and boxes: 0 */
    float verts[KB_MAX_OBJECTS][KB_MAX_POLY_VERTS][2];  /* body frame (origin), world units; boxes as their 4 SetAsBox vertices */
} kb_outline;
int kb_get_outline(const kb_sim *sim, kb_outline *out);
int kb_sense_objects(kb_sim *sim, float *d_obj, float *d_wall, void *stream);

/* Top-down occupancy grids on the CURRENT poses, without stepping: a fixed-size image of the table of every env -- where the
 * kilobots are, which way they face, where each object lies -- for a CENTRAL observer that watches the whole table and moves
 * the light (KilobotsEnv.get_observation, yaml_kilobots_env.py:149-192).  No reference counterpart.  The arena is cut into
 * gw x gh equal cells; row iy = 0 is the ymin edge, column ix = 0 the xmin edge.  Every operation below is one fp32 operation
 * rounded on its own, with correctly rounded divisions:
 *   Host constants: (xmin, xmax, ymin, ymax) = kb_outline.arena;  cw = (xmax - xmin) / (float)gw, icw = (float)gw / (xmax - xmin);
 *     ch = (ymax - ymin) / (float)gh, ich = (float)gh / (ymax - ymin): one subtraction and one division each.
 *   Cell of kilobot i:  tx = (x_i - xmin) * icw;  ix = 0 if !(tx > 0) (NaN included), gw - 1 if tx >= (float)gw, otherwise
 *     (int)tx (truncation);  iy likewise from y_i, ymin, ich and gh.  A kilobot outside the arena lands in the nearest edge
 *     cell, so the count plane of an env always sums to exactly num_bots.
 *   KB_GRID_COUNT, 1 channel: the number of kilobots of the env in the cell, as (float) of the integer (at most 1024: exact).
 *   KB_GRID_FLOW, 2 channels: with (s, c) = the library's sine and cosine of theta_i (the Cephes algorithm every kernel
 *     uses), qc and qs = the fixed-point images of c and s at scale 65536 exactly as KB_REDUCE_SUM quantises a broadcast value
 *     (t = v * 65536; q = 0 if t is NaN, otherwise (int32) rint(clamp(t, -2^21, 2^21)), round half to even);  acc = the int32
 *     sum of qc (first channel), of qs (second channel) over the kilobots of the cell (1024 * 2^16 = 2^26: no overflow);
 *     out = (float)acc / 65536.0f: int -> float to nearest even, then one division.  No two floats are ever added: the result
 *     does not depend on the order of the kilobots.  A heading that is not finite contributes whatever the library's sine and
 *     cosine give for it, and a NaN among them counts as 0.
 *   KB_GRID_OBJECTS, num_objects channels: channel m is 1.0f at cell (iy, ix) if the cell centre
 *     cx = xmin + ((float)ix + 0.5f) * cw, cy = ymin + ((float)iy + 0.5f) * ch  is inside ANY fixture of object m, else 0.0f.
 *     The predicate is the inside flag of kb_sense_objects, taken over unchanged: in the frame (so, co) of otheta_m a polygon
 *     or box fixture covers the centre iff cr >= 0 on all of its edges, a circle iff !(g > 0); the fixtures are those of
 *     kb_get_outline.  It is the fourth word of kb_sense_objects' row for a kilobot whose centre is the cell centre.
 * d_out [num_envs][C][gh][gw] float32, float aligned; C = kb_grid_channels: the channels of the selected planes in the order
 *       count, flow-cos, flow-sin, object 0 .. num_objects - 1.
 * planes: a non-empty subset of KB_GRID_COUNT | KB_GRID_FLOW | KB_GRID_OBJECTS;  1 <= gw, gh <= KB_GRID_MAX_SIDE.
 * Argument errors are reported before an unbound handle, in this order: NULL sim / d_out;  planes;  gw, gh;  KB_GRID_OBJECTS on
 * a handle with num_objects == 0.  Only then comes KB_ENOTBOUND.
 * Reads x, y, theta, ox, oy, otheta; writes d_out only: every element on every call, zeros included (d_out need not be
 * cleared).  At most two launches, none for planes that were not asked for.  Asynchronous on `stream`.
 *
 * kb_grid_channels: C for this handle and these planes, or KB_EINVAL (NULL sim, planes not such a subset, KB_GRID_OBJECTS
 * without objects).  Host only: needs no device and no bound buffers. */
#define KB_GRID_COUNT   1   /* 1 channel: kilobots per cell */
#define KB_GRID_FLOW    2   /* 2 channels: per cell the sum of cos(theta), then of sin(theta) */
#define KB_GRID_OBJECTS 4   /* num_objects channels: cell centre covered by object m */
#define KB_GRID_MAX_SIDE 128
int kb_grid_channels(const kb_sim *sim, int planes);
int kb_sense_grid(kb_sim *sim, int gw, int gh, int planes, float *d_out, void *stream);

/* Nearest-kilobot fields on the CURRENT poses, without stepping: for every cell centre of a gw x gh grid over the arena, which
 * kilobot of the env is nearest and how far away it is -- the Voronoi partition of the table among the kilobots, the cell of
 * every kilobot with its area and its centroid (the target of Lloyd's coverage control), the locational cost and the
 * worst-covered point.  No reference counterpart.  One launch; asynchronous on `stream`.  Every operation below is one fp32
 * operation rounded on its own, with correctly rounded divisions and square roots:
 *   Host constants: those of the occupancy grids above: (xmin, xmax, ymin, ymax) = kb_outline.arena;  cw = (xmax - xmin) / (float)gw,
 *     ch = (ymax - ymin) / (float)gh.  The centre of cell (iy, ix):  cx = xmin + ((float)ix + 0.5f) * cw,
 *     cy = ymin + ((float)iy + 0.5f) * ch  (the formula of KB_GRID_OBJECTS); row iy = 0 is the ymin edge.
 *   Candidates: the kilobots b of the env with d_select[e][b] != 0 (bytes, the convention of d_seed and d_env_mask); NULL: all
 *     of them.  A kilobot outside the arena takes part with its true position.
 *   Per cell: ex = x_b - cx, ey = y_b - cy, d2 = ex * ex + ey * ey.  The owner is the candidate with the smallest
 *     (bits of d2 compared as unsigned integers, b): ties go to the lower index, and nothing else decides it.
 *   d_owner [num_envs][gh][gw] int32: the owner's index within its env.
 *   d_dist  [num_envs][gh][gw] float32: sqrt(d2 of the owner) / 25, metres.
 *   d_cell  [num_envs][num_bots][4] float32, 16-byte aligned: the Voronoi cell of kilobot b on this grid.  n = the number of
 *     cells it owns, SX = the sum of ix and SY = the sum of iy over them (int32; at most 16384 * 127 < 2^24, so (float)SX is
 *     exact), D = the largest d2 among them (the maximum of the bit patterns).  With n > 0:
 *     mx = xmin + (((float)SX / (float)n) + 0.5f) * cw, my likewise from SY, ymin and ch;  dx = mx - x_b, dy = my - y_b;
 *     (s, c) = the library's sine and cosine of theta_b;  the row is ((c * dx + s * dy) / 25, (c * dy - s * dx) / 25, (float)n,
 *     sqrt(D) / 25): the centroid of the cell ahead and to the left in metres, its area in cells, its radius in metres.  With
 *     n == 0, or for a kilobot that is not a candidate: four +0.0f.
 *   d_stats [num_envs][2] float32.  Word 0, the locational cost: q = (int64) rint(min(d2 of the owner * 65536.0f, 0x1p40f)),
 *     round half to even;  acc = the int64 sum of q over the cells;  the word is ((float)acc / 65536.0f) / 625.0f, square
 *     metres summed over the cells (int -> float to nearest even): exact on the quantised values and independent of any order.
 *     The caller scales it by the area of a cell or divides it by gw * gh.  Word 1: sqrt(the largest d2 of an owner) / 25, the
 *     distance of the worst-covered cell centre in metres.
 *   An env without a candidate: d_owner = -1 and d_dist = +inf everywhere, its d_cell rows are zero, its d_stats (+inf, +inf).
 * Each output may be NULL and is then not computed; every element of every output given is written on every call, by a plain
 * store (nothing needs clearing beforehand).  1 <= gw, gh <= KB_GRID_MAX_SIDE.
 * Argument errors are reported before an unbound handle, in this order: NULL sim;  gw, gh;  all four outputs NULL;  a d_cell
 * that is not 16-byte aligned.  Only then comes KB_ENOTBOUND.
 * Reads x, y and d_select, theta only with d_cell; writes the outputs only.  The result of an env does not depend on the other
 * envs.  Poses are assumed finite: with one that is not, the result of its env is unspecified (the call still ends and writes
 * nothing but the outputs). */
int kb_sense_coverage(kb_sim *sim, int gw, int gh, const uint8_t *d_select, int32_t *d_owner, float *d_dist, float *d_cell,
                      float *d_stats, void *stream);

/* Pheromone fields: a grid of floats per env and channel that the kilobots write to and read from, and that diffuses and
 * decays between the steps -- the medium of stigmergy (trails, "food" and "home" pheromones, area marking, quorum sensing by a
 * decaying marker), as the augmented-reality Kilobot tables provide it.  The only sensing entry that carries state across
 * steps: the state is d_field, a tensor the CALLER owns and that this call updates IN PLACE; nothing of it lives in the handle.
 * No reference counterpart (the reference declares a SmoothGridLight and never implements it).  One launch; asynchronous on
 * `stream`.  The grid is that of kb_sense_grid: gw x gh equal cells over the arena, row iy = 0 at ymin, column ix = 0 at xmin.
 * Every operation below is one fp32 operation rounded on its own, nothing is contracted, divisions are correctly rounded.
 * Per selected env and channel c, in this order:
 *   Host constants: those of kb_sense_grid: (xmin, xmax, ymin, ymax) = kb_outline.arena;  icw = (float)gw / (xmax - xmin),
 *     ich = (float)gh / (ymax - ymin);  and hicw = 0.5f * icw, hich = 0.5f * ich.
 *   Cell of kilobot i: (ix, iy) exactly by the rule of kb_sense_grid (clamped to the edge cells, NaN to 0, truncation).
 *   Deposit, only with d_amount != NULL:  a = d_amount[e][i][c];  t = a * 65536.0f;  q = 0 if t is NaN, otherwise
 *     (int32) rint(clamp(t, -2^20, 2^20)), round half to even;  acc = the int32 sum of q over the kilobots of the cell
 *     (1024 * 2^20 = 2^30: no overflow);  dep = (float)acc / 65536.0f (int -> float to nearest even, one division);
 *     u = F + dep for EVERY cell of the plane F (a cell nobody stands in adds +0.0f).  No two floats of different kilobots are
 *     ever added: the result does not depend on their order.  With d_amount == NULL no addition takes place at all, dep is
 *     +0.0f and the bits of F pass through, a -0.0f included.
 *   Iteration, n_iters times, each from the plane u of the one before:  W, E, S, N = the four neighbours of the cell (columns
 *     ix - 1, ix + 1, rows iy - 1, iy + 1), one outside the grid replaced by the cell's own value (a zero-flux edge);
 *     lap = ((W + E) + (S + N)) - 4.0f * u;  v = u + spread[c] * lap;  u' = keep[c] * v.
 *     keep[c] in [0, 1], spread[c] in [0, 0.25]; NaN is rejected.
 *   Sense, only with d_sense != NULL, on the final plane G at the kilobot's cell:  val = G[iy][ix];
 *     dx = (G[iy][min(ix + 1, gw - 1)] - G[iy][max(ix - 1, 0)]) * hicw * 25.0f, evaluated left to right;  dy likewise along the
 *     rows (iy + 1 above iy - 1) with hich;  (s, c) = the library's sine and cosine of theta_i;  the row is
 *     (val, c * dx + s * dy, c * dy - s * dx, dep of the cell): the value, its gradient per metre ahead and to the left, and what
 *     the cell received in this call.
 * d_field  [num_envs][n_channels][gh][gw] float32, float aligned: read and, unless the call is a pure read, written.
 * d_amount [num_envs][num_bots][n_channels] float32, or NULL.
 * d_sense  [num_envs][num_bots][n_channels][4] float32, 16-byte aligned, or NULL.
 * d_env_mask [num_envs] bytes, non-zero = selected, NULL = all (the convention of kb_step_envs).  Of an env that is not selected
 *   no byte of d_field or d_sense is written.
 * keep, spread: HOST arrays [n_channels], read before the call returns.
 * With d_amount == NULL and n_iters == 0 the call is a pure read: d_field is not written at all.
 * The field and the amounts are assumed finite, apart from a NaN amount, which counts as 0; with a field value that is not
 * finite the result of that env and channel is unspecified (the call still ends and writes nothing else).
 * 1 <= gw, gh <= KB_GRID_MAX_SIDE;  1 <= n_channels <= KB_FIELD_MAX_CHANNELS;  0 <= n_iters <= KB_FIELD_MAX_ITERS.
 * Argument errors are reported before an unbound handle, in this order: NULL sim;  gw, gh;  n_channels;  NULL keep / spread or a
 * value out of range;  n_iters;  NULL d_field;  nothing to do (d_amount and d_sense NULL with n_iters == 0);  a d_sense that is
 * not 16-byte aligned.  Only then comes KB_ENOTBOUND.
 * Reads x, y, theta, d_amount and d_env_mask; writes d_field and d_sense only, and no bound buffer. */
#define KB_FIELD_MAX_CHANNELS 4
#define KB_FIELD_MAX_ITERS    64
int kb_field_step(kb_sim *sim, int gw, int gh, int n_channels, const float *keep, const float *spread, int n_iters,
                  const uint8_t *d_env_mask, const float *d_amount, float *d_field, float *d_sense, void *stream);

/* Obstacle-aware distance-to-goal fields on the CURRENT poses, without stepping: the shortest-path distance of every cell of a
 * gw x gh grid over the arena to the nearest goal cell when the objects on the table (and any cells the caller marks) cannot
 * be crossed, the direction of descent per cell, and for every kilobot how far it still has to go and which way, in its own
 * frame -- what a scripted pusher follows to get BEHIND a box, and the "metres still to go" a reward is shaped with.  No
 * reference counterpart.  One launch; asynchronous on `stream`.  Every fp32 operation below is rounded on its own, nothing is
 * contracted, divisions and square roots are correctly rounded.  The distances themselves are integers: the result does not
 * depend on the order in which the kernel relaxes the cells.
 *   Grid: that of kb_sense_grid.  Host constants: (xmin, xmax, ymin, ymax) = kb_outline.arena;  cw = (xmax - xmin) / (float)gw,
 *     icw = (float)gw / (xmax - xmin);  ch, ich likewise from ymin, ymax and gh.  Row iy = 0 is the ymin edge.  The centre of cell
 *     (iy, ix) is that of KB_GRID_OBJECTS: cx = xmin + ((float)ix + 0.5f) * cw, cy = ymin + ((float)iy + 0.5f) * ch.  The cell of a
 *     kilobot is that of KB_GRID_COUNT: clamped to the edge cells, NaN to 0, truncation.
 *   Step costs (host; kb_path_costs returns them):  q(l) = (int32) rint(min(max(l * 1024.0f, 1.0f), 65536.0f));  qx = q(cw),
 *     qy = q(ch), qd = q(dg) with dg = sqrt(cw * cw + ch * ch).  Directions k = 0..7 are (dx, dy) = (1,0), (1,1), (0,1), (-1,1),
 *     (-1,0), (-1,-1), (0,-1), (1,-1);  w_k = qx for k in {0, 4}, qy for k in {2, 6}, qd for odd k.  A shortest path visits a
 *     cell at most once: a finite distance is below 16384 * 65536 = 2^30 and D + w fits int32.  "No path" is never added to.
 *   Blocked cells: cell c is blocked iff d_blocked[e][iy][ix] != 0 (NULL blocks none);  or, for an object m with bit m of
 *     `objects` set, the cell centre is inside ANY fixture of m (the inside flag of kb_sense_objects, taken over unchanged);
 *     or, with clear_m > 0 and for such an object, !(d2 > C2), where d2 is the squared distance of the winning candidate of
 *     kb_sense_objects for a kilobot standing on the cell centre and Cw = clear_m * 25.0f, C2 = Cw * Cw (host).  With
 *     clear_m == 0 the d2 test is not made: the object part is exactly the OR of the selected KB_GRID_OBJECTS planes.
 *   Moves: from a free cell a to its neighbour b in direction k iff b is inside the grid and free and, for odd k, both
 *     (ax + dx, ay) and (ax, ay + dy) are free as well -- no cutting of corners, no squeezing between two obstacles that touch
 *     diagonally.  The relation is symmetric.
 *   Sources: cell c is a source iff d_source[e][iy][ix] != 0 and c is free.
 *   Distance: D(c) of a free cell is the least sum of w_k along allowed moves from any source, 0 at a source, "none" without a
 *     path.  D is unique.
 *   d_dist [num_envs][gh][gw] float32: ((float)D / 1024.0f) / 25.0f metres for a reached cell (int -> float to nearest even);
 *     +inf for a blocked cell and for a free cell without a path.
 *   d_next [num_envs][gh][gw] int8: for a reached cell that is no source the lowest k with an allowed move to b and
 *     D(b) + w_k == D(c);  -1 at a source, -2 at a free cell without a path, -3 at a blocked cell.
 *   d_bot  [num_envs][num_bots][4] float32, 16-byte aligned.  For kilobot i in its cell c:  c free and reached: Db = D(c),
 *     kb = next(c).  c blocked (a kilobot pressing on an object stands inside the clearance band: the normal case for a
 *     pusher): the candidates are the directions k whose neighbour b is inside the grid, free and reached -- no corner rule --
 *     with the value D(b) + w_k; the least value wins, ties go to the lowest k, Db and kb are the winner's.  Otherwise the
 *     kilobot is unreachable.  Unit vectors (host): (ux, uy) = ((float)dx, (float)dy) for even k and ((float)dx * (cw / dg),
 *     (float)dy * (ch / dg)) for odd k.  With (s, c) = the library's sine and cosine of theta_i the row is
 *     (((float)Db / 1024.0f) / 25.0f, c * ux + s * uy, c * uy - s * ux, flag);  the direction words are +0.0f at a source and
 *     when unreachable;  flag = 0.0f for a free reached cell, 1.0f for a source cell, 2.0f for a blocked cell with a way out,
 *     3.0f for unreachable, whose distance is +inf.
 *   d_stats [num_envs][4] float32.  Word 0: the number of kilobots with a finite Db.  Word 1: ((float)(the int64 sum of those
 *     Db) / 1024.0f) / 25.0f, the swarm's metres to go, independent of any order.  Word 2: the largest such Db in metres as
 *     above, +0.0f with none.  Word 3: the number of free cells reached, sources included.
 * d_source, d_blocked [num_envs][gh][gw] bytes, non-zero = set (the convention of d_seed and d_env_mask); d_blocked may be NULL.
 * Each output may be NULL and is then neither computed nor written; every element of every output given is written on every
 * call, by a plain store.  1 <= gw, gh <= KB_GRID_MAX_SIDE;  0 <= objects < 2^num_objects;  clear_m >= 0 and finite.
 * Argument errors are reported before an unbound handle, in this order: NULL sim / d_source;  gw, gh;  objects;  clear_m;  all
 * four outputs NULL;  a d_bot that is not 16-byte aligned.  Only then comes KB_ENOTBOUND.
 * Reads x, y (theta only with d_bot), ox, oy, otheta (only with objects != 0), d_source and d_blocked; writes the outputs only,
 * and no bound buffer.  The result of an env does not depend on the other envs.  Poses are assumed finite apart from what the
 * cell rule says of a NaN.
 *
 * kb_path_costs: out = (qx, qy, qd) for this handle's arena and this grid, or KB_EINVAL (NULL argument; gw, gh).  Host only:
 * needs no device and no bound buffers. */
int kb_path_costs(const kb_sim *sim, int gw, int gh, int32_t *out /* host, [3]: qx, qy, qd */);
int kb_sense_paths(kb_sim *sim, int gw, int gh, const uint8_t *d_source, const uint8_t *d_blocked, int objects, float clear_m,
                   float *d_dist, int8_t *d_next, float *d_bot, float *d_stats, void *stream);

/* Kilobot-to-slot matching on the CURRENT poses, without stepping: the two-sided nearest-neighbour query of shape formation
 * between the kilobots of an env and the K points ("slots") of a target shape -- for every kilobot the nearest slot in its own
 * frame, for every slot the nearest kilobot (which slots are still free), whether a kilobot holds the slot it is nearest to,
 * and per env the two directed Chamfer sums, the two directed Hausdorff distances and the fill counts a reward is made of.
 * No reference counterpart.  One launch; asynchronous on `stream`.  Every operation below is one fp32 operation rounded on
 * its own, nothing is contracted, divisions and square roots are correctly rounded:
 *   d_points: [num_envs][K][2] float32 with per_env != 0, [K][2] shared by all envs with per_env == 0; METRES;  K = n_targets,
 *     1 <= K <= KB_MAX_TARGETS.  Slot t in world units: tx = px * 25.0f, ty = py * 25.0f, one multiplication each, on the device.
 *   Sides: the kilobots b of the env with d_bot_select[e][b] != 0 and the slots t with d_slot_select[e][t] != 0 (bytes, the
 *     convention of d_select, d_seed and d_env_mask); NULL: all of them.  d_bot_select is [num_envs][num_bots], d_slot_select
 *     always [num_envs][K], also with shared points.  A kilobot outside the arena takes part with its true position, and so
 *     does a slot outside it.
 *   One distance serves both directions: ex = tx - x_b, ey = ty - y_b, d2(b, t) = ex * ex + ey * ey.
 *   Host constants: Tw = tol_m * 25.0f, T2 = Tw * Tw (as kb_sense takes R2);  tol_m >= 0 and finite.  "Within tolerance" is
 *     !(d2 > T2).
 *   Kilobot to slot.  A selected kilobot b gets the selected slot with the smallest (bits of d2(b, t) compared as unsigned
 *     integers, t): ties go to the lower slot index, and nothing else decides it.
 *     d_index [num_envs][num_bots] int32: that t.
 *     d_rel   [num_envs][num_bots][4] float32, 16-byte aligned: with (s, c) = the library's sine and cosine of theta_b and ex,
 *       ey, d2 those of (b, t) the row is ((c * ex + s * ey) / 25, (c * ey - s * ex) / 25, sqrt(d2) / 25, mutual): the slot ahead
 *       and to the left in metres, its distance in metres, and mutual = 1.0f iff b is the owner (below) of t, else 0.0f.
 *     A kilobot that is not selected: d_index = -1 and four +0.0f.  A selected kilobot in an env without a selected slot:
 *     d_index = -1 and (+0.0f, +0.0f, +inf, +0.0f).
 *   Slot to kilobot.  A selected slot t gets the selected kilobot with the smallest (bits of d2(b, t), b): its owner.
 *     d_owner [num_envs][K] int32: that b.
 *     d_dist  [num_envs][K] float32: sqrt(d2) / 25, metres.
 *     A slot that is not selected: -1 and +0.0f.  A selected slot in an env without a selected kilobot: -1 and +inf.
 *   d_stats [num_envs][6] float32.  Words 0 and 2, the directed Chamfer sums: over the selected kilobots of d2 to their slot
 *     (word 0) and over the selected slots of d2 to their owner (word 2), the fixed-point sum of word 0 of kb_sense_coverage:
 *     q = (int64) rint(min(d2 * 65536.0f, 0x1p40f)), round half to even;  acc = the int64 sum of q;  the word is
 *     ((float)acc / 65536.0f) / 625.0f, square metres (int -> float to nearest even): independent of any order.  Words 1 and
 *     3, the directed Hausdorff distances: sqrt(the largest such d2) / 25, the maximum of the bit patterns.  Word 4: the
 *     number of selected slots whose owner is within tolerance (filled slots);  word 5: the number of selected kilobots whose
 *     slot is within tolerance;  both (float) of the integer.  With either side of the env empty words 0..3 are +inf and words
 *     4 and 5 are +0.0f.
 * Each output may be NULL and is then neither computed for its own sake nor written; every element of every output given is
 * written on every call, by a plain store (nothing needs clearing beforehand).  mutual and the stats are right whatever else
 * was asked for.
 * Argument errors are reported before an unbound handle, in this order: NULL sim or NULL d_points;  n_targets;  tol_m;  all five
 * outputs NULL;  a d_rel that is not 16-byte aligned.  Only then comes KB_ENOTBOUND.
 * Reads x, y, d_points and the two selections, theta only with d_rel; writes the outputs only, and no bound buffer.  The result
 * of an env does not depend on the other envs.  Poses and points are assumed finite: with one that is not, the result of its
 * env is unspecified (the call still ends and writes nothing but the outputs). */
#define KB_MAX_TARGETS 1024
int kb_sense_targets(kb_sim *sim, const float *d_points, int n_targets, int per_env, float tol_m, const uint8_t *d_bot_select,
                     const uint8_t *d_slot_select, int32_t *d_index, float *d_rel, int32_t *d_owner, float *d_dist,
                     float *d_stats, void *stream);

/* One-to-one kilobot-to-slot matching on the CURRENT poses, without stepping: the GREEDY (locally dominant) matching between the
 * kilobots of an env and the K slots of a target shape -- who goes where, which slots stay free, and the sums a formation
 * reward is made of -- where kb_sense_targets gives the two nearest queries, in which twenty kilobots may all name one slot.
 * No reference counterpart.  One launch; asynchronous on `stream`.  It is not the optimal assignment.
 * Points, sides, d2(b, t), T2 and the shapes and alignment of the five outputs are exactly those of kb_sense_targets; every
 * operation is one fp32 operation rounded on its own.
 *   Cutoff: Cw = cutoff_m * 25.0f, C2 = Cw * Cw;  cutoff_m >= 0, +inf allowed (C2 = +inf: no cutoff); a NaN or a negative
 *     value is KB_EINVAL.  A pair (b, t) is ADMISSIBLE if b and t are selected and !(d2(b, t) > C2).
 *   Total order on pairs: (bits of d2 compared as unsigned integers, b, t), lexicographic.  Nothing else decides anything.
 *   The matching M: walk the admissible pairs of the env in ascending order and take a pair iff neither its kilobot nor its
 *     slot has been taken.  M is unique.
 *   Rounds: R is the number of rounds of this process -- among the still unmatched selected entries every kilobot chooses the
 *     admissible slot with the least (bits of d2, t) and every slot the admissible kilobot with the least (bits of d2, b);
 *     pairs that choose each other are matched at once; repeat until no admissible pair is left.  The process yields M (a pair
 *     that is the least at both its ends is exactly a pair the walk takes), every round with an admissible pair matches at
 *     least the least one, so R <= min(selected kilobots, selected slots).  R is a property of the scene.
 *   d_index [num_envs][num_bots] int32: the slot matched to b, or -1.
 *   d_rel   [num_envs][num_bots][4] float32, 16-byte aligned: for a matched b, with (s, c), ex, ey, d2 as in kb_sense_targets,
 *     ((c * ex + s * ey) / 25, (c * ey - s * ex) / 25, sqrt(d2) / 25, 1.0f).  Selected but unmatched: (+0.0f, +0.0f, +inf,
 *     +0.0f).  Not selected: four +0.0f.
 *   d_owner [num_envs][K] int32, d_dist [num_envs][K] float32: the kilobot matched to t and sqrt(d2) / 25.  Selected but
 *     unmatched: -1 and +inf.  Not selected: -1 and +0.0f.
 *   d_stats [num_envs][6] float32, over the pairs of M.  Word 0: the fixed-point sum of d2, exactly word 0 of kb_sense_targets
 *     (q = (int64) rint(min(d2 * 65536.0f, 0x1p40f)), the int64 sum acc, ((float)acc / 65536.0f) / 625.0f), square metres.
 *     Word 1: sqrt(the largest bits of d2) / 25, the bottleneck distance.  Word 2: the fixed-point sum of the distances,
 *     dm = sqrt(d2) / 25.0f, q = (int64) rint(min(dm * 65536.0f, 0x1p40f)), the int64 sum acc, (float)acc / 65536.0f, metres.
 *     Word 3: (float)R.  Word 4: the number of pairs with !(d2 > T2).  Word 5: (float)|M|.  With no pair all six are +0.0f.
 * Each output may be NULL and is then not written; every element of every output given is written on every call, by a plain
 * store.
 * Argument errors are reported before an unbound handle, in this order: NULL sim or NULL d_points;  n_targets;  tol_m;
 * cutoff_m;  all five outputs NULL;  a d_rel that is not 16-byte aligned.  Only then comes KB_ENOTBOUND.
 * Reads x, y, d_points and the two selections, theta only with d_rel; writes the outputs only, and no bound buffer.  The result
 * of an env does not depend on the other envs.  Poses and points are assumed finite, as for kb_sense_targets. */
int kb_sense_assign(kb_sim *sim, const float *d_points, int n_targets, int per_env, float tol_m, float cutoff_m,
                    const uint8_t *d_bot_select, const uint8_t *d_slot_select, int32_t *d_index, float *d_rel, int32_t *d_owner,
                    float *d_dist, float *d_stats, void *stream);

/* Touch and push sensing from the contact store, without stepping: who touches whom, and how hard -- what the solver alone
 * knows (Body.collides_with, body.py:87-90, walks b2Body.contacts; the impulses have no reference counterpart).  A pure
 * function of ws_key / ws_acc / ws_cnt as the last kb_step left them: the Box2D contact list of the last world step.
 *   Store reading, env e, N = num_bots, M = num_objects, cap = kb_contact_capacity():  off[a] = sum of ws_cnt[e][b], b < a;
 *     entry (a, s), s < ws_cnt[e][a], sits at pos = off[a] + s and is skipped when pos >= cap (never stored);
 *     key = ws_key[e][pos], acc = ws_acc[e][pos].
 *   Meaning of an entry of owner a, by key:
 *     key < N, key != a: a kilobot-kilobot contact.  It is stored under ONE of its two kilobots (not always the lower) and is
 *       reported in the list of a with code key and in the list of key with code a.
 *     0x10000 <= key < 0x10004: a wall.  The store numbers walls 0 xmin, 1 ymin, 2 xmax, 3 ymax; the public index is that of
 *       kb_sense_objects (0 xmin, 1 xmax, 2 ymin, 3 ymax): W = (0, 2, 1, 3)[key - 0x10000], code N + W.
 *     key >= 0x20000, f = key - 0x20000 < fixtures of the handle: fixture f in the kb_config numbering (NOT the body-grouped
 *       order of kb_outline), of object m = obj_fixture_body[f] (f when num_fixtures == 0): code N + 4 + m, sub-order f.
 *     Every other key is ignored.
 *   Order of a kilobot's list: ascending by the 64-bit key ((code * 8 + f) << 32) | bits(acc), f = 0 unless a fixture:
 *     kilobots first, then walls, then objects with fixtures ascending -- whatever order the store holds.
 * d_partner [num_envs][num_bots][k] int32 and d_impulse [num_envs][num_bots][k] float32, both or neither, 1 <= k <=
 *       KB_MAX_CONTACT_SLOTS: the first min(k, count) entries of the list, the code and acc with unchanged bits; unused slots
 *       hold -1 and +0.0.
 * d_touch [num_envs][num_bots][4] float32 or NULL: kilobot contacts, wall contacts, fixture contacts, impulse sum -- over ALL
 *       entries of the kilobot, never truncated by k.  The sum is the fixed-point sum of kb_sense_reduce:
 *       (float)(int32)(sum of q(acc)) / scale with q the quantisation of KB_REDUCE_SUM, accumulated modulo 2^32: exact on the
 *       quantised values and independent of the order.
 * d_obj [num_envs][num_objects][2] float32 or NULL: the kilobot-fixture contacts on object m and the same fixed-point sum of
 *       their impulses.  KB_EINVAL on a handle without objects.
 * scale: finite and > 0; 65536 resolves 1.5e-5 over +-32 (impulses are in Box2D world units: b2ManifoldPoint::normalImpulse
 *       after the velocity iterations of the last substep).
 * Meaningful when the env's status has bit 0 clear; the list is that of the contacts the last world step found on the poses
 * BEFORE its integration (as after b2World::Step); stale after poses were set without a step; empty once ws_cnt is zeroed;
 * after the resolve step of a reset it lists the overlaps with impulse 0 (count and flags still report them).
 * Argument errors are reported before an unbound handle, in this order: NULL sim;  exactly one of d_partner / d_impulse;  k
 * (when the lists are asked for);  scale;  all outputs NULL;  d_obj without objects.  Only then comes KB_ENOTBOUND.
 * Reads ws_key, ws_acc, ws_cnt; may use the env's slice of kb_buffers.scratch (transient by contract); writes the outputs
 * only, every element of every output given on every call.  One launch.  Asynchronous on `stream`. */
#define KB_MAX_CONTACT_SLOTS 16
int kb_sense_contacts(kb_sim *sim, int k, float scale, int32_t *d_partner, float *d_impulse, float *d_touch, float *d_obj,
                      void *stream);

/* RGB frames of every env, rasterised on the device: what KilobotsEnv.render draws (kilobots_env.py:221-275 with
 * Kilobot.draw, kilobot.py:129-145, Body.draw, body.py:156-281, and Light.draw, light.py:95-96,194-195) as a point-sampled
 * image with every operation stated.  No pixel parity with pygame is claimed: its integer circle and line rasterisers are
 * not restated.  A pure function of the poses, the object poses and the light positions; no range cut, no state.
 * d_rgb [num_envs][height][width][3] uint8, R, G, B; row 0 is the ymax edge (the viewer flips y), column 0 the xmin edge;
 *       byte aligned.  Every byte is written on every call, exactly once, by a plain store.
 * d_body_rgb, d_mark_rgb [num_envs][num_bots] uint32 words 0x00RRGGBB (the top byte is ignored) or NULL: the body colour and
 *       the colour of the heading mark (the LED) of every kilobot (Kilobot._body_color, _highlight_color; set_color,
 *       kilobot.py:83-84,262-263).  NULL: style->body / style->mark for every kilobot.
 * style NULL: the defaults of kb_render_default_style, the reference's colours: table (255, 255, 255) kilobots_env.py:252-253,
 *       body (150, 150, 150) kilobot.py:42,132, ring (100, 100, 100) kilobot.py:133, mark (255, 255, 255) kilobot.py:43,145,
 *       light (255, 255, 30) with light_alpha 150 light.py:195, every obj[m] (93, 133, 195) body.py:21.
 * Host constants, all fp32, every step one operation rounded on its own:  (xmin, xmax, ymin, ymax) = kb_outline.arena;
 *   cw = (xmax - xmin) / (float)width, ch = (ymax - ymin) / (float)height;  with r = bot_radius:  ro = r + 0.002f,
 *   Ro = ro * 25.0f, Ro2 = Ro * Ro, Ri = (ro - 0.005f) * 25.0f, Ri2 = Ri * Ri, Lf = (r - 0.005f) * 25.0f, Hw = 0.0025f * 25.0f;
 *   per positional light component l:  Rl = radius_l * 25.0f, Rl2 = Rl * Rl  (radius_l: light_radius, or lightc_radius[l]
 *   of a composite light).
 * Pixel (row j, column i); every multiplication, addition and comparison is its own fp32 operation, nothing is contracted:
 *   px = xmin + ((float)i + 0.5f) * cw,  py = ymin + ((float)(height - 1 - j) + 0.5f) * ch;  the colour starts as table.
 *   KB_RENDER_OBJECTS: obj[m] of the HIGHEST m whose inside flag holds for the point (px, py) (painter's order,
 *     kilobots_env.py:261-262); the flag is the predicate of kb_sense_objects / KB_GRID_OBJECTS, unchanged.  The highlight
 *     triangle of a CornerQuad (body.py:174) is not drawn: the handle does not know a CornerQuad from a Quad.
 *   KB_RENDER_BOTS: for kilobot b  qx = px - x_b, qy = py - y_b, dd = qx * qx + qy * qy;  b covers the pixel iff dd <= Ro2 (a NaN
 *     or infinite coordinate never covers).  The HIGHEST covering b wins (painter's order, kilobots_env.py:265-266); no other
 *     kilobot matters.  With (s, c) the library's sine and cosine of theta_b, a = c * qx + s * qy, l = c * qy - s * qx:
 *       mark_b  if Lf > 0 && a >= 0 && a <= Lf && fabsf(l) <= Hw  (the line from the centre to the front, kilobot.py:137-145),
 *       ring    otherwise if !(Ri > 0) || dd > Ri2  (the 5 mm outline, kilobot.py:133-134),
 *       body_b  otherwise.  A kilobot pixel replaces the object colour.
 *   KB_RENDER_LIGHT: last, for every positional component l in component order (KB_LIGHT_CIRCULAR and KB_LIGHT_MOMENTUM, alone
 *     or inside a KB_LIGHT_COMPOSITE):  fx = light_x[e][l] * 25.0f - px, fy likewise;  inside iff fx * fx + fy * fy <= Rl2.  An
 *     inside pixel is blended per channel in integers, v = (light_c * A + v * (255 - A) + 127) / 255 with A = light_alpha; later
 *     components blend over earlier ones.  A handle with no light or a KB_LIGHT_GRADIENT light draws nothing for this layer:
 *     not an error.
 *   The arena border line (kilobots_env.py:254-255, 3 mm wide, centred on the edge) is not drawn.
 * Argument errors are reported before an unbound handle, in this order: NULL sim / d_rgb;  layers not a non-empty subset of
 * the three bits;  width or height outside 1..KB_RENDER_MAX_SIDE.  Only then comes KB_ENOTBOUND.
 * Reads x, y, theta; ox, oy, otheta when the handle has objects and the layer is on; light_x, light_y when it has positional
 * lights and the layer is on; the two colour arrays when given.  Writes d_rgb only.  One launch.  Asynchronous on `stream`.
 *
 * kb_render_default_style: the defaults into *out; KB_EINVAL for NULL.  Host only. */
#define KB_RENDER_OBJECTS 1
#define KB_RENDER_BOTS    2
#define KB_RENDER_LIGHT   4
#define KB_RENDER_MAX_SIDE 2048
typedef struct kb_render_style {
    uint8_t table[3], body[3], ring[3], mark[3], light[3], light_alpha;
    uint8_t obj[KB_MAX_OBJECTS][3];
} kb_render_style;
int kb_render_default_style(kb_render_style *out);
int kb_render(kb_sim *sim, int width, int height, int layers, const kb_render_style *style,
              const uint32_t *d_body_rgb, const uint32_t *d_mark_rgb, uint8_t *d_rgb, void *stream);

/* Range scans on the CURRENT poses, without stepping: for every kilobot i and each of n_rays bearings in its own frame, how
 * far the first thing in that direction is and what it is -- another kilobot, a pushable object or a wall: the occlusion-aware,
 * fixed-size observation of decentralised navigation and pushing policies.  A body hidden behind another is not seen.  The
 * result of an env does not depend on the other envs of the batch.  No reference counterpart.  Every operation below is one
 * fp32 operation rounded on its own, nothing is contracted, divisions and square roots are correctly rounded; all lengths
 * are world units until the final / 25:
 *   Host constants:  Rw = radius_m * 25;  rb = bot_radius * 25, rb2 = rb * rb;  Rc = Rw + rb, Rc2 = Rc * Rc.
 *   Directions:  u_k = ((float)cos(2 pi k / n_rays), (float)sin(2 pi k / n_rays)), k = 0 .. n_rays - 1, evaluated in double and
 *     rounded to fp32; the entries at whole quarter turns (4 k a multiple of n_rays) are exactly (+-1, 0) and (0, +-1).  Ray 0
 *     points dead ahead, the rays run counter-clockwise.  kb_ray_directions writes this very table, the one the kernel is
 *     handed, into xy (HOST memory, [n_rays][2]); it needs no handle and no device, and returns KB_EINVAL for an n_rays outside
 *     1..KB_MAX_RAYS or a NULL xy.
 *   Body frame of kilobot i:  (s, c) = the library's sine and cosine of theta_i (the Cephes algorithm every kernel uses).  A
 *     world point P becomes  dx = P.x - x_i, dy = P.y - y_i;  a = c * dx + s * dy (ahead), l = c * dy - s * dx (to the left).
 *     For the point (a, l) and ray k:  b = a * u.x + l * u.y (along the ray),  q = a * u.y - l * u.x (across it).
 *   Disc of radius r, r2 = r * r, with its centre as the point:  h2 = r2 - q * q;  a miss if !(h2 >= 0);  sq = sqrt(h2),
 *     t1 = b - sq, t2 = b + sq;  a miss if !(t2 >= 0);  t = t1 >= 0 ? t1 : t2 -- the first crossing of the outline at t >= 0:
 *     from inside a disc that is the way out.
 *   Segment from vertex A to vertex B, with (bA, qA) and (bB, qB):  it straddles the ray iff (qA <= 0 && qB >= 0) ||
 *     (qA >= 0 && qB <= 0);  den = qA - qB;  a miss if den == 0;  sg = qA / den,  t = bA + sg * (bB - bA);  a miss if !(t >= 0).
 *   Every candidate is a hit iff t <= Rw;  then t = t > 0 ? t : +0.0f.
 *   Candidates:
 *     KB_RAY_BOTS: the kilobots j != i of the env with !(dd > Rc2), ex = x_j - x_i, ey = y_j - y_i, dd = ex * ex + ey * ey (the
 *       predicate of kb_sense at the radius Rw + rb); each a disc with r2 = rb2 at (x_j, y_j), code j.
 *     KB_RAY_OBJECTS: every fixture of every object of kb_get_outline, no range cut.  With (so, co) the sine and cosine of
 *       otheta_m, a circle fixture is a disc of radius[f] (r2 = radius[f] * radius[f]) at (ox_m, oy_m); a polygon or box
 *       fixture gives the segments v[k] -> v[(k + 1) % n] between its world vertices  wx = ox_m + (co * vx - so * vy),
 *       wy = oy_m + (so * vx + co * vy).  Code num_bots + 4 + m.  On a body with several fixtures (LForm, TForm, CForm) a
 *       kilobot whose centre is inside the body may report an interior edge, where two fixtures meet -- the caveat of
 *       kb_sense_objects.
 *     KB_RAY_WALLS: the four segments of kb_outline.arena, in this vertex order:  W0 (xmin, ymin) -> (xmin, ymax),
 *       W1 (xmax, ymin) -> (xmax, ymax),  W2 (xmin, ymin) -> (xmax, ymin),  W3 (xmin, ymax) -> (xmax, ymax).  Code num_bots + W:
 *       the wall numbering of kb_sense_objects.  A kilobot outside the arena sees the walls from behind.
 *   Per ray the hit with the smallest (t, code) wins: bits(t) compared as unsigned, then the code -- whatever order the
 *     candidates are met in.  A ray through a shared vertex hits both edges at the same t up to rounding.
 * d_dist [num_envs][num_bots][n_rays] float32: t / 25, metres; Rw / 25 where nothing was hit.
 * d_hit  [num_envs][num_bots][n_rays] int32 or NULL: the winner's code (the codes of kb_sense_contacts), -1 where nothing was hit.
 * targets: a non-empty subset of KB_RAY_BOTS | KB_RAY_OBJECTS | KB_RAY_WALLS;  1 <= n_rays <= KB_MAX_RAYS;  radius_m > 0 (a
 * radius beyond the arena is fine).  Argument errors are reported before an unbound handle, in this order: NULL sim / d_dist;
 * targets;  n_rays;  radius_m;  KB_RAY_OBJECTS on a handle with num_objects == 0.  Only then comes KB_ENOTBOUND.
 * Reads x, y, theta, and ox, oy, otheta with KB_RAY_OBJECTS; writes the two outputs only, every element on every call, by
 * plain stores.  One launch.  Asynchronous on `stream`. */
#define KB_RAY_BOTS    1
#define KB_RAY_OBJECTS 2
#define KB_RAY_WALLS   4
#define KB_MAX_RAYS    32
int kb_ray_directions(int n_rays, float *xy /* host, [n_rays][2] */);
int kb_sense_rays(kb_sim *sim, float radius_m, int n_rays, int targets, float *d_dist, int32_t *d_hit, void *stream);

/* The sensing point of ONE substep on its own, for kilobots that are programmed on the host (a Kilobot subclass with its
 * own _loop, kilobot.py:86-88,164-168): Light.step with d_light_action ([num_envs][kb_light_action_dim()], NULL = action None:
 * the light stays) and value_and_gradients at every kilobot's light sensor (kilobots_env.py:171-180) into
 * kb_buffers.light_value / light_gx / light_gy, exactly the arithmetic the fused step uses.  The host then runs the
 * kilobots' _loop (get_ambientlight -> light_value, set_motors -> motor_l / motor_r) and calls
 * kb_step(sim, NULL, NULL, 1, 0, stream): motor law + world.Step of that substep (the light is not stepped again). */
int kb_light_sense(kb_sim *sim, const float *d_light_action, void *stream);

/* KilobotsEnv.reset() for every env of the handle, on the device (kilobots_env.py:150-159 with the spawn rule of
 * YamlKilobotsEnv._init_kilobots, yaml_kilobots_env.py:346-352): positions ~ N(mean, std) per coordinate, clipped to
 * the world bounds -/+ 0.02 m, theta = 0 (body.py:28-29) or U(-pi, pi); commands and accelerations zeroed
 * (random_velocity: the U([0, 0.01] x [-pi/2, pi/2]) initial command of kilobot.py:225-229); motors as after
 * Kilobot._setup -> turn_left; phototaxis counters cleared; warm-start impulses forgotten; status cleared.  Object
 * and light state is not touched.  resolve != 0 appends the "step to resolve" of kilobots_env.py:156-157 (one world.Step
 * with the kilobots at rest).
 * Random numbers: Philox4x32-10, key = seed (lo, hi), counter = (env_offset + env, bot, 0, 0); the four outputs give the
 * two Box-Muller normals, the heading and the command.  A shard created with env_offset = its first global env index
 * reproduces the corresponding rows of the unsharded reset bit for bit (the reference itself is not reproducible:
 * seed() only stores the number, kilobots_env.py:145-148). */
typedef struct kb_reset_params {
    uint64_t seed;
    int32_t env_offset;
    float mean[2];          /* metres */
    float std;              /* metres */
    int32_t random_theta;
    int32_t random_velocity;
    int32_t resolve;
} kb_reset_params;
int kb_reset(kb_sim *sim, const kb_reset_params *rp, void *stream);

/* KilobotsEnv.reset() for the envs a mask selects, on the device: one env ends its episode and starts the next while the
 * others run on.  d_env_mask as for kb_step_envs.  For a selected env e:
 *   - exactly the writes kb_reset makes to the rows of env e, with the Philox counter (env_offset + e, bot, z, 0),
 *     z = d_episode[e], or 0 when d_episode (or init) is NULL: then the rows equal those of a full kb_reset with the same rp
 *     bit for bit.  A caller that counts the episodes of every env in d_episode makes the j-th episode of global env e a pure
 *     function of (seed, e, j), whenever the other envs end and however the batch is sharded;
 *   - d_obj_pose: ox, oy, otheta are copied bitwise, ovx, ovy, ow set to 0, osleep to 0 when bound (Body.__init__,
 *     body.py:32-38); the env's ows_acc is forgotten as kb_reset already does;
 *   - d_light_pos: light_x, light_y are copied; light_vx, light_vy come from d_light_vel, or are 0 when that is NULL and the
 *     buffers are bound.  (d_light_vel alone sets the velocities only.)
 *   - rp->resolve != 0 appends kb_step_envs(sim, d_env_mask, NULL, NULL, 1, KB_STEP_NO_DRIVE, stream): at most two launches.
 * For an unselected env no byte of any bound buffer changes (kb_buffers.scratch excluded, as for kb_step_envs).
 * Argument checks in this order: NULL sim, rp or mask -> KB_EINVAL;  std not >= 0 -> KB_EINVAL;  d_obj_pose on a handle with
 * num_objects == 0, d_light_pos or d_light_vel on a handle without a light -> KB_EINVAL;  an unbound handle -> KB_ENOTBOUND.
 * Random object and light placement is the caller's: it supplies per-env templates, which it can randomise in torch. */
typedef struct kb_episode_init {            /* every member optional (NULL) */
    const uint32_t *d_episode;   /* [num_envs]: word z of the Philox counter of env e; NULL = 0 (the draw of kb_reset) */
    const float *d_obj_pose;     /* [num_envs][num_objects][3]: ox, oy (world units, as stored), otheta */
    const float *d_light_pos;    /* [num_envs][kb_light_count()][2]: light_x, light_y as stored (GradientLight: angle in [0]) */
    const float *d_light_vel;    /* [num_envs][kb_light_count()][2]: light_vx, light_vy */
} kb_episode_init;
int kb_reset_envs(kb_sim *sim, const kb_reset_params *rp, const uint8_t *d_env_mask,
                  const kb_episode_init *init /* may be NULL */, void *stream);

/* KilobotsEnv.get_state()['kilobots'] (kilobots_env.py:115-118 -> body.py:63-72):
 * d_out [num_envs][num_bots][3] = (x [m], y [m], theta). */
int kb_get_poses(kb_sim *sim, float *d_out, void *stream);

/* The whole of KilobotsEnv.get_state() of the kilobots and objects (kilobots_env.py:115-118 -> body.py:63-72) and the
 * status word in ONE buffer, for hosts that read the state back after every step (one copy instead of three):
 * d_out [num_envs][3 num_bots + 3 num_objects + 1] float32 = per env the kilobots' (x [m], y [m], theta), the objects'
 * (x [m], y [m], theta), then the bit pattern of the env's int32 kb_buffers.status word. */
int kb_get_state(kb_sim *sim, float *d_out, void *stream);

/* Introspection */
int kb_lds_bytes(const kb_sim *sim);            /* dynamic LDS per workgroup (one env per workgroup) */
int kb_light_action_dim(const kb_sim *sim);     /* floats per env in d_light_action */
int kb_light_count(const kb_sim *sim);          /* light components per env (0 without a light) */
int kb_contact_capacity(const kb_sim *sim);     /* contacts (and warm-start entries) per env */
int kb_lds_staging_entries(const kb_sim *sim);  /* contacts of one env that are staged in LDS; an env with more takes its slice of
                                                   kb_buffers.scratch for that substep (same results, slower).  kb_create trades
                                                   entries for resident envs per CU, never below num_bots + 64 (at
                                                   least 128) up to 512 kilobots without objects, 688 above 512, and
                                                   5 num_bots / 2 + 64 (at least 256) with objects or mixed drive laws */
size_t kb_scratch_bytes(const kb_sim *sim);     /* size of kb_buffers.scratch: 32 B per contact of the capacity (staging record; level-sorted record of the cooperative sweeps) */
int kb_block_threads(const kb_sim *sim);
int kb_variant_index(const kb_sim *sim);        /* which instantiation of the step kernel runs the handle: its position in the library's
                                                   list (kb_variant.h: kb_variants), -1 if the library has none (kb_step then fails).
                                                   Follows kb_set_block_threads.  For tests that must know which kernel they ran */
int kb_exact_division(const kb_sim *sim);       /* 1: the position sweep of the register solver takes -C / K by multiplying with RN(1 / K) (one
                                                   correction step, same bits): kb_create compared the form with the division for this handle's
                                                   two K, over every mantissa of the dividend in the binade of the largest |C| (0.2), every
                                                   1021st mantissa in each smaller binade down to 2^-34, and both zeros.  0: it divides */
int kb_exact_selftest(const kb_sim *sim, unsigned long long *d_counts, void *stream);
                                                /* for tests: the short forms of the position sweep (square root, reciprocal, division by this
                                                   handle's two K) with the device's own seed instructions against the compiler's IEEE sequences
                                                   over all 2^32 bit patterns.  d_counts (device, 6 words): per form the operands inside its
                                                   guard and the results that differ in a bit */
int kb_debug_lds(int mode, uint32_t word, unsigned long long *d_count, void *stream);
                                                /* for tests: one small kernel on twice as many workgroups as the current device has CUs, each
                                                   with the full 160 KiB of LDS.  mode 0 stores `word` into every LDS word (d_count unused, may be
                                                   NULL); mode 1 stores nothing and counts into d_count[0] (device, 2 words, zeroed first) the LDS
                                                   words equal to `word`, into d_count[1] the words looked at: what a kernel finds of its
                                                   predecessor's LDS.  Another mode, or mode 1 without d_count -> KB_EINVAL.  Asynchronous */
int kb_resident_envs_per_cu(kb_sim *sim);        /* workgroups (= envs) of this handle's kernel that one CU holds at a time (HIP occupancy query; needs a GPU) */
int kb_set_block_threads(kb_sim *sim, int threads);  /* multiple of 64 in [64, 512], num_bots <= 2 * threads.  kb_create picks
                                                         the measured best (one kilobot per thread, power-of-two wave count,
                                                         as many resident envs as the LDS allows); results never depend on
                                                         it.  kb_lds_bytes() follows (tables sized by the wave count). */
const char *kb_last_error(void);
const char *kb_version(void);

#ifdef __cplusplus
}
#endif
#endif
