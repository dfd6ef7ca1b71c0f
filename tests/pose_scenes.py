"""Objects and poses of the pose tests (tests/test_pose_host.py, tests/test_gpu_pose.py) over the scenes of tests/refit_scenes.py.

Scene A as 34 objects: the floor (2 triangles), 32 cubes (12 each), the sphere (320).  A pose of scene A: every cube its own rotation, shear (up to
0.2) and non-uniform scale (0.5 .. 1.5) about its own centre plus a translation (up to 0.3 per axis); the floor stretched and shifted; the sphere
MIRRORED, scaled and turned about its centre -- the mirror only there: the sphere has no quad or box leaves.  tests/test_pose_host.py checks on
the CPU that every cube of the posed scene still passes the builders' box rule and every quad leaf the quad rule."""
import numpy as np

from tests import refit_scenes as RS

N_OBJECTS_A = 2 + RS.N_CUBES


def scene_a_first():
    """The object table of scene A: n_objects + 1 first triangles."""
    return np.array([0, RS.FLOOR_TRIS] + [RS.cube_first_triangle(i) + 12 for i in range(RS.N_CUBES)] + [RS.FLOOR_TRIS + RS.CUBE_TRIS + RS.SPHERE_TRIS], np.uint32)


def _about(A, centre, shift):
    """[A | t] with t such that `centre` goes to centre + shift."""
    c = np.asarray(centre, np.float64)
    return np.concatenate([A, (c - A @ c + np.asarray(shift, np.float64))[:, None]], axis=1)


def identity(n_objects):
    return np.tile(np.eye(3, 4, dtype=np.float32).reshape(1, 12), (n_objects, 1))


def scene_a_xforms(seed, rest=None):
    """[34, 12] float32: a pose of scene A (see above), a function of the seed.  rest: the buffers the objects' centres are taken from (scene_a(0))."""
    rest = RS.scene_a(0) if rest is None else rest
    P = rest["positions"][rest["indices"]].astype(np.float64)
    first = scene_a_first()
    rng = np.random.default_rng(7000 + seed)
    M = np.zeros((N_OBJECTS_A, 3, 4))
    M[0] = _about(np.diag([1.1, 1.0, 0.95]), (0, 0, 0), (0.05, 0.0, -0.03))
    for i in range(RS.N_CUBES):
        centre = P[3 * first[1 + i]:3 * first[2 + i]].mean(0)
        S = np.eye(3)
        a, b = rng.choice(3, 2, replace=False)
        S[a, b] = rng.uniform(-0.2, 0.2)
        A = RS._rot(rng.normal(size=3), rng.uniform(-0.6, 0.6)) @ S @ np.diag(rng.uniform(0.5, 1.5, 3))
        M[1 + i] = _about(A, centre, rng.uniform(-0.3, 0.3, 3) * np.array([1.0, 0.3, 1.0]))
    A = RS._rot(rng.normal(size=3), rng.uniform(-0.5, 0.5)) @ np.diag([-1.0, 1.0, 1.0]) * rng.uniform(0.7, 1.3)
    M[-1] = _about(A, RS.SPHERE_CENTER, rng.uniform(-0.1, 0.1, 3))
    return np.ascontiguousarray(M.reshape(N_OBJECTS_A, 12).astype(np.float32))


def posed_buffers(b, pos, nrm):
    """The buffer dict `b` with posed positions (and normals, if any)."""
    return dict(b, positions=pos, normals=b["normals"] if nrm is None else nrm)


# the tables trg_pose_bind refuses for scene A (706 triangles), by name; the last two need the INDEXED scene A, whose triangles share vertices
def bad_tables():
    good = scene_a_first()
    order = good.copy()
    order[5], order[6] = good[6], good[5]
    end = good.copy()
    end[-1] = 700
    split_sphere = np.concatenate([good[:-1], [good[-2] + 100], good[-1:]]).astype(np.uint32)
    one_triangle = np.concatenate([[0, 1], good[1:]]).astype(np.uint32)
    return {"not ascending": (order, False), "not ending at n_tris": (end, False), "a vertex shared by two objects": (split_sphere, True),
            "an object of one triangle": (one_triangle, True)}
