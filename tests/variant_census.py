"""The census of the step-kernel instantiations: tests/golden/variant_census.txt has one configuration per entry of
kb_variants (gym_kilobots_amd/csrc/kb_variant.h) -- the smallest shape that selects it and still has contacts -- and this
module turns a row into a scene: config keywords, poses, objects and the inputs of every substep.  Shared by
tests/test_variant_census_cpu.py (the table maps one to one onto the list; no scene is vacuous on the oracle) and
tests/test_variant_census_gpu.py (every instantiation runs its scene bit for bit against the oracle)."""
import os
import subprocess
from types import SimpleNamespace

import numpy as np

from oracle import oracle as O
from tests import scenes
from tests.scenes import put_numpy  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CENSUS = os.path.join(ROOT, 'tests', 'golden', 'variant_census.txt')
NUM_VARIANTS = 176

# prints kb_variants, then for every input row of stdin (the columns of tests/golden/launch_plan.txt) the status of
# plan_launch and the position of the selected instantiation in the list
PROGRAM = r'''
#include <cstdio>
#include "kb_launch.h"
using namespace kb;
int main() {
    for (int i = 0; i < kb_variants.n; ++i) {
        const Variant &k = kb_variants.v[i];
        printf("%d %d %d %d %d %d %d %d\n", k.drive, k.light, k.obj, k.fn, k.tier, k.poly, k.sense, k.sleep);
    }
    printf("--\n");
    int v[11];
    while (scanf("%d %d %d %d %d %d %d %d %d %d %d", &v[0], &v[1], &v[2], &v[3], &v[4], &v[5], &v[6], &v[7], &v[8], &v[9], &v[10]) == 11) {
        const Plan p = plan_launch({v[0], v[1], v[2], v[3] != 0, v[4], v[5], v[6] != 0, v[7] != 0, v[8], v[9], v[10]});
        printf("%d %d\n", p.status, p.status == KB_OK ? variant_index(p.variant) : -1);
    }
    return 0;
}
'''


def host_census(workdir, inputs):
    """Compile kb_launch.h with the system compiler and run `inputs` (lists of the eleven plan inputs) through plan_launch:
    (the library's list as tuples of eight ints, [(status, index) per input])."""
    src = os.path.join(str(workdir), 'census.cpp')
    exe = os.path.join(str(workdir), 'census')
    with open(src, 'w') as f:
        f.write(PROGRAM)
    subprocess.check_call(['g++', '-std=c++17', '-I', os.path.join(ROOT, 'include'), '-I', os.path.join(ROOT, 'gym_kilobots_amd', 'csrc'),
                           src, '-o', exe])
    stdin = '\n'.join(' '.join(map(str, r)) for r in inputs).encode()
    out = subprocess.run([exe], input=stdin, stdout=subprocess.PIPE, check=True).stdout.decode().split('\n')
    sep = out.index('--')
    listed = [tuple(int(x) for x in l.split()) for l in out[:sep]]
    selected = [tuple(int(x) for x in l.split()) for l in out[sep + 1:sep + 1 + len(inputs)]]
    return listed, selected


def rows():
    """[(inputs, index, variant)] of the committed table: the eleven plan inputs, the position it must select, and the
    template arguments of that instantiation (drive, light, obj, fn, tier, poly, sense, sleep)."""
    out = []
    for line in open(CENSUS):
        if line.startswith('#') or not line.strip():
            continue
        inputs, index, variant = line.split(':')
        out.append(([int(x) for x in inputs.split()], int(index), tuple(int(x) for x in variant.split())))
    return out


DRIVE_NAMES = ['velocity', 'accel', 'motors', 'simplephoto', 'photo', 'mixed']
LIGHT_NAMES = {O.LIGHT_NONE: 'nolight', O.LIGHT_CIRCULAR: 'circular', 99: 'general'}
LIGHT_MODEL_NAMES = ['nolight', 'circular', 'gradient', 'momentum', 'composite']


def row_id(row):
    """e.g. 017-accel-general-gradient-boxes-t0-sleep, 160-velocity-nolight-fixed1024-nosense-sleep"""
    inputs, index, (drive, light, obj, fn, tier, poly, sense, sleep) = row
    parts = ['%03d' % index, DRIVE_NAMES[drive], LIGHT_NAMES[light]]
    if light == 99:
        parts.append(LIGHT_MODEL_NAMES[inputs[5]])
    if inputs[1] > 0:
        parts.append('boxes' if poly else 'discs')
    parts.append('fixed1024' if fn else 't%d' % tier)
    if not sense:
        parts.append('nosense')
    if sleep:
        parts.append('sleep')
    return '-'.join(parts)


def stop_and_go_actions(E, N, k, seed):
    """Velocity commands in which groups of kilobots stop for a while (they fall asleep in their islands) and start again."""
    rng = np.random.RandomState(seed + k)
    a = scenes.random_actions(E, N, seed=seed + 100 + k)
    phase = (np.arange(N)[None, :] // 7 + np.arange(E)[:, None] + k // 9) % 3
    a[phase == 0] = 0.0                                   # a third of the kilobots rests for 9 substeps at a time
    a[rng.rand(E, N) < 0.05] = 0.0
    return a.astype(np.float32)


E = 2
SINGLE_SUBSTEPS, FUSED_SUBSTEPS = 45, 10
SENSE_RADIUS = 0.07
OBJECTS = np.array([[0.1, 0.05], [-0.15, -0.1]])
FAR_OBJECT = np.array([-0.7, 0.5])          # phototaxis rows: the second object rests apart from the swarm and falls asleep
LIGHT_BOUNDS = dict(light_lo=(-1.1, -0.825), light_hi=(1.1, 0.825))

CIRCULAR_FIELDS = ('light_x', 'light_y', 'light_value', 'light_gx', 'light_gy')
GENERAL_FIELDS = ('light_x', 'light_y', 'light_vx', 'light_vy', 'light_value', 'light_gx', 'light_gy')
PHOTOTAXIS_FIELDS = ('motor_l', 'motor_r', 'pt_threshold', 'pt_update', 'pt_nochange', 'pt_dir')
OBJ_FIELDS = ('ox', 'oy', 'otheta', 'ovx', 'ovy', 'ow', 'ows_acc')


def _light_kw(light, resting):
    """Bounds and radii of tests/test_parity_gpu.py (test_light_driven_modes, test_other_light_models).  resting: the
    SimplePhototaxis rows with the sleep state take lights so small that part of the swarm lies outside them -- a
    kilobot outside every radius senses a zero gradient, is commanded (0, 0) and falls asleep."""
    if light == O.LIGHT_CIRCULAR:
        return dict(light_radius=0.1 if resting else 0.4, **LIGHT_BOUNDS)
    if light == O.LIGHT_MOMENTUM:
        return dict(light_radius=0.1 if resting else 0.5, light_max_velocity=0.01, **LIGHT_BOUNDS)
    if light == O.LIGHT_COMPOSITE:
        b = LIGHT_BOUNDS
        return dict(light_count=3, light_kind=[O.LIGHT_CIRCULAR, O.LIGHT_MOMENTUM, O.LIGHT_CIRCULAR],
                    lightc_radius=[0.1, 0.12, 0.08] if resting else [0.3, 0.4, 0.25], lightc_max_velocity=[np.inf, 0.008, np.inf],
                    lightc_lo=[b['light_lo']] * 3 + [(0, 0)], lightc_hi=[b['light_hi']] * 3 + [(0, 0)])
    return {}


def spawn(N, seed_shift=0):
    """The poses of every row with N kilobots; seed_shift != 0: the twin scene of tests/guarded.py, the same spawn rule with
    another seed."""
    if N == 1024:
        return scenes.lattice_spawn(E, N, seed=7 + seed_shift)
    return scenes.gaussian_spawn(E, N, sigma=0.05 + 0.0004 * N, seed=N + seed_shift)


def scene(row):
    """Everything a run of one census row needs:
      E, N, mode, light, kw     arguments of tests.gpu_common.make_pair / oracle.default_config
      block_threads             what to ask of kb_set_block_threads (0: keep kb_create's width)
      xy, th                    kilobot poses
      objects, ovx              object positions and their velocity at the start (None without objects)
      state                     {buffer name: array} written into both sims before the first substep (motors, laws, lights, ...)
      steps                     [(n_substeps, actions or None, light_action or None)]: 45 single substeps, one fused launch of 10
      fields                    what is compared bit for bit after every launch
      sleeps                    sleep rows: True if kilobots must fall asleep on the oracle, False if the drive law keeps all of
                                them moving for the whole scene (asserted either way by the CPU test); None without sleep state
      objects_sleep             phototaxis sleep rows with objects: an object must fall asleep"""
    inputs, index, (drive, lclass, obj, fn, tier, poly, sense, sleep) = row
    N, M, _, discs, mode, light, sense_on, allow_sleep, _, capacity, threads = inputs
    rng = np.random.RandomState(9000 + index)
    s = SimpleNamespace(E=E, N=N, mode=mode, light=light, block_threads=threads, index=index, state={}, objects=None, ovx=None,
                        sleeps=None, objects_sleep=False)
    phototaxis = mode in (O.DRIVE_SIMPLE_PHOTOTAXIS, O.DRIVE_PHOTOTAXIS)
    kw = dict(allow_sleep=allow_sleep, contact_capacity=capacity, sense_radius=SENSE_RADIUS if sense_on else 0.0)
    kw.update(_light_kw(light, resting=bool(allow_sleep) and mode == O.DRIVE_SIMPLE_PHOTOTAXIS))
    if mode == O.DRIVE_MIXED:
        kw.update(mode_density=[2.0, 2.0, 1.0, 1.0, 1.0])
    if M:
        kw.update(num_objects=M)
        if not discs:       # 0.15 x 0.10 m boxes (half extents in world units)
            kw.update(obj_shape=[O.SHAPE_BOX] * M + [0] * (8 - M), obj_nverts=[4] * M + [0] * (8 - M),
                      obj_verts=[[[0.075 * 25.0, 0.05 * 25.0]] + [[0.0, 0.0]] * 3] * M + [[[0.0, 0.0]] * 4] * (8 - M))
        s.objects = np.tile(OBJECTS[None, :M], (E, 1, 1))
        s.ovx = np.full((E, M), 4.0, np.float32)
        if phototaxis:
            s.objects[:, 1] = FAR_OBJECT
            s.ovx[:, 1] = 0.0
            s.objects_sleep = bool(allow_sleep)
    s.kw = kw
    s.xy, s.th = spawn(N)

    # state before the first substep
    if mode in (O.DRIVE_MOTORS, O.DRIVE_MIXED):
        ml, mr = rng.randint(0, 256, (E, N)).astype(np.uint8), rng.randint(0, 256, (E, N)).astype(np.uint8)
        off = rng.rand(E, N) < 0.35         # switched off: these kilobots rest
        ml[off] = 0
        mr[off] = 0
        s.state.update(motor_l=ml, motor_r=mr)
    if mode == O.DRIVE_MIXED:
        s.state.update(bot_mode=rng.randint(0, 5, (E, N)).astype(np.uint8))
    if mode == O.DRIVE_PHOTOTAXIS:
        # a kilobot program that has not started yet: motors off, a threshold no measurement exceeds.  It rests until the
        # counter of unchanged measurements reaches 15 (kilobot.py:318-333): at the check of substep 36 for a start value of 9
        # (the kilobot wakes up inside the scene), not within the scene for 0.  The other kilobots run the reference's _setup
        off = rng.rand(E, N) < 0.35
        late = off & (rng.rand(E, N) < 0.5)
        ml, mr = np.full((E, N), 255, np.uint8), np.zeros((E, N), np.uint8)
        ml[off] = 0
        thr = np.full((E, N), -np.inf, np.float32)
        thr[off] = np.inf
        noch = np.zeros((E, N), np.int32)
        noch[late] = 9
        s.state.update(motor_l=ml, motor_r=mr, pt_threshold=thr, pt_nochange=noch)
    if light != O.LIGHT_NONE:
        LC = 3 if light == O.LIGHT_COMPOSITE else 1
        shape = (E,) if LC == 1 else (E, LC)
        s.state.update(light_x=rng.uniform(-0.2, 0.2, shape).astype(np.float32))
        if light != O.LIGHT_GRADIENT:
            s.state.update(light_y=rng.uniform(-0.2, 0.2, shape).astype(np.float32))
        if light in (O.LIGHT_MOMENTUM, O.LIGHT_COMPOSITE):
            v0 = rng.uniform(-0.005, 0.005, shape).astype(np.float32)
            s.state.update(light_vx=v0, light_vy=-v0)

    # inputs of every launch
    adim = {O.LIGHT_NONE: 0, O.LIGHT_GRADIENT: 1, O.LIGHT_COMPOSITE: 6}.get(light, 2)
    takes_actions = mode in (O.DRIVE_VELOCITY, O.DRIVE_ACCEL, O.DRIVE_MIXED)
    s.steps = []
    for k in range(SINGLE_SUBSTEPS + 1):
        a = stop_and_go_actions(E, N, k, seed=7) if takes_actions else None
        la = None if adim == 0 or k % 3 == 2 else rng.uniform(-0.02, 0.02, (E, adim)).astype(np.float32)
        s.steps.append((1 if k < SINGLE_SUBSTEPS else FUSED_SUBSTEPS, a, la))

    s.fields = ('x', 'y', 'theta', 'cmd_vx', 'cmd_vy', 'cmd_w')
    if takes_actions:
        s.fields += ('v', 'w')
    if mode in (O.DRIVE_PHOTOTAXIS, O.DRIVE_MIXED):
        s.fields += PHOTOTAXIS_FIELDS
    if light == O.LIGHT_CIRCULAR:
        s.fields += CIRCULAR_FIELDS
    elif light != O.LIGHT_NONE:
        s.fields += GENERAL_FIELDS
    if M:
        s.fields += OBJ_FIELDS
    if allow_sleep:
        s.fields += ('sleep_time',) + (('osleep',) if M else ())
        # a GradientLight has the same non-zero gradient everywhere: SimplePhototaxis kilobots never rest under it
        s.sleeps = not (mode == O.DRIVE_SIMPLE_PHOTOTAXIS and light == O.LIGHT_GRADIENT)
    if sense_on:
        s.fields += ('nbr_count',)
    return s


def apply_start(s, sim, put):
    """Objects and start state of scene s into one sim (poses are set by make_pair / set_poses_m before);
    put(sim, name, array) writes one buffer."""
    if s.objects is not None:
        sim.set_objects_m(s.objects)
        put(sim, 'ovx', s.ovx)
    for name, val in s.state.items():
        put(sim, name, val)


def oracle_sim(s):
    osim = O.OracleSim(O.default_config(s.E, s.N, s.mode, s.light, **s.kw))
    osim.set_poses_m(s.xy, s.th)
    apply_start(s, osim, put_numpy)
    return osim


def oracle_step(osim, step):
    n, a, la = step
    if a is not None:
        osim.set_actions(a)
    osim.step(n, light_action=la)
