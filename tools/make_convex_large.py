"""Writes the large convex test hulls (tests/golden/meshes/{blob100,prism18,prism44}.stl, binary test vectors; tests/golden/convex_large.xml reads them from there; needs scipy for the hulls) from seeded numpy.

The convex narrow phase runs one wavefront per geom pair and spreads vertices, faces, edges and polygon points over its 64 lanes; the
bundled hulls (box, tetrahedron, pyramid, dodecahedron) never take such a loop past its first trip.  These three do:

* ``blob100``: hull of 100 seeded points on an ellipsoid with semi-axes 0.11 / 0.08 / 0.06 -- 100 vertices, 196 triangles, 294 edges,
  3 vertices per face; irregular, so generic poses have no exact index ties;
* ``prism18``: right prism over a slightly irregular 18-gon -- 36 vertices, 20 faces, 54 edges, 18 vertices per face (the 4-vertex side
  faces are padded to 18);
* ``prism44``: right prism over a slightly irregular 44-gon -- 88 vertices; its caps exceed the 20-vertex face limit and are subsampled
  (every third vertex, 15 of 44), so the faces do not name every vertex of the hull.

``python tools/make_convex_large.py`` rewrites the three files; ``ellipsoid_points`` / ``hull_triangles`` / ``write_stl`` are what tests/test_convex_large.py uses to
make a hull too large for the pair kernel in a temporary directory.
"""
import os
import struct

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MESHES = os.path.join(ROOT, "tests", "golden", "meshes")

BLOB_SEED, BLOB_N, BLOB_AXES = 100, 100, (0.11, 0.08, 0.06)
PRISM_SEED = 18


def ellipsoid_points(n, axes=BLOB_AXES, seed=BLOB_SEED):
    """n seeded points on an ellipsoid: every one of them is a vertex of their hull."""
    u = np.random.RandomState(seed).randn(n, 3)
    return u / np.linalg.norm(u, axis=1, keepdims=True) * np.asarray(axes, dtype=np.float64)


def prism_points(n, radius=0.1, half_height=0.05, seed=PRISM_SEED):
    """Right prism over an n-gon inscribed in a circle, the angles jittered by a fifth of their spacing (no two edges parallel by construction)."""
    rng = np.random.RandomState(seed + n)
    ang = 2 * np.pi * (np.arange(n) + 0.2 * rng.uniform(-1, 1, n)) / n
    ring = radius * np.stack([np.cos(ang), np.sin(ang)], axis=1)
    return np.concatenate([np.concatenate([ring, np.full((n, 1), z)], axis=1) for z in (-half_height, half_height)])


def hull_triangles(points):
    """Outward-oriented triangles [T, 3, 3] of the convex hull."""
    from scipy.spatial import ConvexHull

    pts = np.asarray(points, dtype=np.float64)
    hull = ConvexHull(pts)
    tris = pts[hull.simplices]
    flip = np.einsum("ti,ti->t", np.cross(tris[:, 1] - tris[:, 0], tris[:, 2] - tris[:, 0]), hull.equations[:, :3]) < 0
    tris[flip] = tris[flip][:, [0, 2, 1]]
    return tris


def write_stl(path, tris):
    """Binary STL: 80-byte header, triangle count, then normal + three vertices in float32 and a 16-bit attribute per triangle."""
    tris = np.asarray(tris, dtype=np.float64)
    n = np.cross(tris[:, 1] - tris[:, 0], tris[:, 2] - tris[:, 0])
    n = n / np.linalg.norm(n, axis=1, keepdims=True)
    with open(path, "wb") as f:
        f.write(os.path.basename(path).encode().ljust(80, b" "))
        f.write(struct.pack("<I", len(tris)))
        for t, nn in zip(tris, n):
            f.write(struct.pack("<12fH", *nn, *t.reshape(-1), 0))


def main():
    os.makedirs(MESHES, exist_ok=True)
    write_stl(os.path.join(MESHES, "blob100.stl"), hull_triangles(ellipsoid_points(BLOB_N)))
    write_stl(os.path.join(MESHES, "prism18.stl"), hull_triangles(prism_points(18)))
    write_stl(os.path.join(MESHES, "prism44.stl"), hull_triangles(prism_points(44)))
    for n in ("blob100", "prism18", "prism44"):
        print(n, os.path.getsize(os.path.join(MESHES, n + ".stl")), "bytes")


if __name__ == "__main__":
    main()
