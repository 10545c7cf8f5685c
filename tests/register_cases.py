"""The case table of the registration tests, shared by test_register_ref.py (CPU: the table is not vacuous, the
restatement converges) and test_gpu_register.py (GPU: the library against tests/register_ref.py bit for bit).

Scenes are rendered by fuse_cases.render.  The corner scene is fuse_cases.PLANE with a side wall and a floor: three planes whose normals
span space, so all six freedoms of a pose are fixed.  The single plane leaves three of them free: its first step must be refused.  The
source view stands in slot 1 (between its targets), is rendered from the TRUE pose and carries the START pose, which is what the one-shot
entry begins with."""
import functools

import numpy as np

import fuse_cases as fc
import register_ref as rr

SRC = 1
WALL = (np.array([1.0, 0.0, 0.35]) / np.linalg.norm([1.0, 0.0, 0.35]), 2.2)
FLOOR = (np.array([0.0, 1.0, 0.30]) / np.linalg.norm([0.0, 1.0, 0.30]), 1.6)
CORNER = [(fc.PLANE[0], fc.PLANE[1], None), (WALL[0], WALL[1], None), (FLOOR[0], FLOOR[1], None)]
SINGLE = [(fc.PLANE[0], fc.PLANE[1], None)]
TRUE = (fc.rot(1.5, -3.0, 2.0), np.array([0.15, -0.04, 0.1]))
OFF = (fc.rot(1.0, -1.5, 1.0), np.array([0.05, -0.03, 0.04]))
START = (OFF[0] @ TRUE[0], TRUE[1] + OFF[1])
# slots 0, 2, 3: the targets.  Slot 3 stands half a unit forward: a source's near speckles lie behind it.
TARGET_POSES = {0: (np.eye(3), np.zeros(3)), 2: (fc.rot(-1.0, 2.0, -1.5), np.array([-0.2, 0.03, 0.05])), 3: (fc.rot(0.5, 4.0, 1.0), np.array([0.25, -0.02, 0.5]))}


def pose_error(R, t, truth=TRUE):
    """-> (rotation angle in degrees, translation distance) between a pose and the truth"""
    dR = np.asarray(R).reshape(3, 3) @ truth[0].T
    ang = np.degrees(np.arccos(np.clip((np.trace(dR) - 1.0) / 2.0, -1.0, 1.0)))
    return float(ang), float(np.linalg.norm(np.asarray(t) - truth[1]))


@functools.lru_cache(maxsize=None)
def scene(kind, w, h, n_targets, seed=0):
    """-> a tuple of 1 + n_targets view dicts (n_targets 1 or 3), the source in slot SRC.  kind: corner, single (exact renders),
    spoiled (the corner, every view spoiled), huge (the corner; the targets' depths 50 times too large and their normals scaled by
    3e152: the sums b overflow while A stays finite)"""
    rng = np.random.default_rng(1000 * seed + 7 * w + 13 * h + n_targets)
    planes = SINGLE if kind == "single" else CORNER
    slots = [0, SRC] if n_targets == 1 else [0, SRC, 2, 3]
    views = []
    for k in slots:
        R, t = TRUE if k == SRC else TARGET_POSES[k]
        cam = fc.camera(w, h, k, R, t)
        depth, normal, _ = fc.render(cam, w, h, planes)
        if kind == "spoiled":
            fc.spoil(depth, normal, rng, k)
        if kind == "huge" and k != SRC:
            depth, normal = depth * 50.0, normal * 3e152
        if k == SRC:
            cam = dict(cam, R=START[0], t=START[1])
        views.append(fc.view(cam, depth, normal))
    return tuple(views)


class Case:
    def __init__(self, name, w, h, n_targets, kind="spoiled", seed=0, **params):
        self.name, self.w, self.h, self.n_targets, self.kind = name, w, h, n_targets, kind
        self.scene_args = (kind, w, h, n_targets, seed)
        self.params = dict(rr.DEFAULTS, **params)
        self.targets = 0b0001 if n_targets == 1 else 0b1101

    def views(self):
        return list(scene(*self.scene_args))

    def reference(self):
        """register_ref's result (computed once per case and shared; nobody writes into it)"""
        return _reference(self)

    def __repr__(self):
        return self.name


@functools.lru_cache(maxsize=None)
def _reference(case):
    return rr.register(case.views(), case.w, case.h, SRC, case.targets, **case.params)


SHAPES = [(1, 1, 1), (7, 5, 1), (64, 4, 1), (257, 1, 1), (65, 5, 2), (130, 67, 1), (130, 67, 3), (300, 220, 1)]


def _table():
    cases, n = [], 0
    for w, h, stride in SHAPES:
        for n_targets in (1, 3):
            for min_cos in (0.0, 0.9):
                few = w * h < 1000  # the solve runs on the small shapes too
                cases.append(Case(f"{w}x{h}_s{stride}_T{n_targets}_c{min_cos}", w, h, n_targets, seed=n, iters=3, stride=stride, min_cos=min_cos,
                                  **(dict(min_pairs=6) if few else {})))
                n += 1
    return cases


CASES = _table()
# the convergence condition: the exact corner, the default parameters (8 iterations)
CONVERGE = [Case("corner_130x67_s1", 130, 67, 1, kind="corner"), Case("corner_64x48_s2", 64, 48, 1, kind="corner", stride=2)]
SINGLE_PLANE = Case("single_130x67", 130, 67, 1, kind="single")
NONFINITE = Case("huge_7x5", 7, 5, 3, kind="huge", iters=2, max_dist=1e4, huber=0.0, min_pairs=1)
EXTRA = CONVERGE + [SINGLE_PLANE, NONFINITE]
BY_NAME = {c.name: c for c in CASES + EXTRA}
assert len(BY_NAME) == len(CASES) + len(EXTRA)
