"""Build-defined benchmark scenes (BASELINE.json configs 3-5).

config 3: media/cornell-box/scene_specular.json (metal tall box, dielectric short box,
          dielectric sphere).
config 4: `instanced_cubes()` — media/cube.obj (12 triangles) instanced on a jittered 3-D grid
          inside the Cornell box (scale 0.01–0.03, rng seed 1234), walls and light kept:
          83 334 instances + 36 = 1 000 044 triangles.
"""
import os

import numpy as np

from .core.bsdf import BSDF
from .io_utils.read_tungsten import load_obj, read_file

MEDIA = os.path.join(os.path.dirname(os.path.abspath(__file__)), "media")
CORNELL = os.path.join(MEDIA, "cornell-box", "scene.json")
CORNELL_SPECULAR = os.path.join(MEDIA, "cornell-box", "scene_specular.json")


class MeshBatch:
    """Many triangles under one BSDF, world-space already (vectorised TriangleMesh)."""
    type_name = "mesh"

    def __init__(self, vertices, faces, bsdf):
        from .mathematics.bbox import BBox
        self.id = -1
        self.vertices = np.asarray(vertices, np.float64)
        self.faces = np.asarray(faces, np.int64)
        self.bsdf = bsdf
        tri = self.vertices[self.faces]
        e1 = tri[:, 1] - tri[:, 0]
        e2 = tri[:, 2] - tri[:, 0]
        c = np.cross(e1, e2)
        n = np.sqrt(c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1] + c[:, 2] * c[:, 2])
        self.normal_vectors = (c / n[:, None]).astype(np.float32)   # Cube convention: +normalize(e1 x e2)
        self.bounds = BBox(None, None)
        self.bounds.from_vertices(self.vertices)
        self.center = self.bounds.center()

    @property
    def bounding_box(self):
        return self.bounds.min_coord, self.bounds.max_coord


def instanced_cubes(n_instances=83334, seed=1234, scale=(0.01, 0.03), albedo=(0.725, 0.71, 0.68)):
    """Config 4: Cornell box + n_instances jittered, scaled copies of media/cube.obj."""
    scene, cam = read_file(CORNELL)
    v, f = load_obj(os.path.join(MEDIA, "cube.obj"))
    rng = np.random.default_rng(seed)
    g = int(np.ceil(n_instances ** (1.0 / 3.0)))
    cells = np.stack(np.meshgrid(np.arange(g), np.arange(g), np.arange(g), indexing="ij"), -1).reshape(-1, 3)
    cells = cells[rng.permutation(cells.shape[0])[:n_instances]]
    lo = np.array([-0.95, 0.02, -0.95])
    hi = np.array([0.95, 1.90, 0.95])
    size = (hi - lo) / g
    s = rng.uniform(scale[0], scale[1], n_instances)
    origin = lo + (cells + rng.uniform(0.1, 0.9, (n_instances, 3))) * size - 0.5 * s[:, None]
    verts = (v[None, :, :] - 0.0) * s[:, None, None] + origin[:, None, :]          # cube.obj spans [0,1]^3
    faces = f[None, :, :] + (np.arange(n_instances) * v.shape[0])[:, None, None]
    mat = BSDF({"type": "lambert", "albedo": list(albedo)}).get_distribution()
    scene.add_primitive(MeshBatch(verts.reshape(-1, 3), faces.reshape(-1, 3), mat))
    return scene, cam


def _rigid(matrix, what):
    """A 4 x 4 float64 rigid matrix (rotation with determinant +1 and a translation), or a ValueError."""
    g = np.asarray(matrix, np.float64)
    if g.shape != (4, 4) or not np.isfinite(g).all() or not np.array_equal(g[3], (0.0, 0.0, 0.0, 1.0)):
        raise ValueError(f"{what} must be a finite 4 x 4 matrix with the last row (0, 0, 0, 1)")
    r = g[:3, :3]
    if np.abs(r.T @ r - np.eye(3)).max() > 1e-9 or abs(np.linalg.det(r) - 1.0) > 1e-9:
        raise ValueError(f"{what} is not rigid: its 3 x 3 part must be a rotation")
    return g


def spin(prim, degrees):
    """The rigid 4 x 4 matrix that turns `prim` by `degrees` about the vertical (y) axis through the centre of
    its bounding box."""
    lo, hi = prim.bounding_box
    c = 0.5 * (np.asarray(lo, np.float64) + np.asarray(hi, np.float64))
    t = np.radians(degrees)
    g = np.eye(4)
    g[:3, :3] = [[np.cos(t), 0.0, np.sin(t)], [0.0, 1.0, 0.0], [-np.sin(t), 0.0, np.cos(t)]]
    g[:3, 3] = c - g[:3, :3] @ c
    return g


def moved(scene, moves):
    """A new Scene with the primitives listed in `moves` ({index: 4 x 4 rigid matrix}) re-posed: the matrix is
    applied to the primitive's world pose (trans_mat becomes G @ trans_mat, a sphere's centre G applied to it).
    Quad and Cube are rebuilt from the new transform, a TriangleMesh keeps its faces, takes G applied to its world
    vertices and has explicit face normals rotated.  A MeshBatch is rejected with a ValueError: it holds
    world-space triangles of many instances and no transform that pyrenderer_amd.denoise.motion_rows could
    compare.  Every other primitive, and every BSDF object, is shared with `scene`, so flatten_scene's material
    table is unchanged."""
    from .core.scene import Scene
    from .mathematics.shapes import Cube, Quad, Sphere, TriangleMesh, apply_transform
    moves = {int(i): _rigid(g, f"the matrix of primitive {i}") for i, g in dict(moves).items()}
    n = len(scene.primitives)
    for i in moves:
        if not 0 <= i < n:
            raise ValueError(f"no primitive {i}: the scene has {n}")
    out = Scene()
    for i, prim in enumerate(scene.primitives):
        g = moves.get(i)
        if g is None:
            out.add_primitive(prim)
        elif isinstance(prim, Sphere):
            out.add_primitive(Sphere(g[:3, :3] @ prim.center + g[:3, 3], prim.radius, prim.bsdf))
        elif isinstance(prim, (Quad, Cube)):
            out.add_primitive(type(prim)(g @ np.asarray(prim.trans_mat, np.float64), prim.bsdf))
        elif isinstance(prim, TriangleMesh):
            normals = (np.asarray(prim.normal_vectors, np.float64) @ g[:3, :3].T).astype(np.float32)
            vertices, faces = apply_transform(prim.vertices, prim.faces, g)
            new = TriangleMesh(np.eye(4), prim.bsdf, vertices, faces, face_normals=normals)
            new.trans_mat = g @ np.asarray(prim.trans_mat, np.float64)
            out.add_primitive(new)
        else:
            raise ValueError(f"primitive {i} ({type(prim).__name__}) cannot be moved: only Quad, Cube, TriangleMesh "
                             f"and Sphere carry a pose")
    return out


def spun(scene, index, degrees, frames):
    """`frames` scenes: `scene` itself, then each the one before with primitive `index` turned by `degrees` about
    the vertical axis through the centre of its bounding box in `scene` (the same axis for every frame)."""
    if not 0 <= int(index) < len(scene.primitives):
        raise ValueError(f"no primitive {index}: the scene has {len(scene.primitives)}")
    g = spin(scene.primitives[int(index)], degrees)
    out = [scene]
    for _ in range(1, int(frames)):
        out.append(moved(out[-1], {int(index): g}))
    return out
