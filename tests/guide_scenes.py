"""The scenes of tests/test_hits_gpu.py and tests/test_guides_gpu.py, as text: each test loads its scene
with DeviceScene.from_text, so that material ids are the text's -- the reference span lists' and the
oracle's -- and tests/precompile_guides.py compiles the guides module of exactly these texts."""
import os
import re

import numpy as np

import zoo as T
from pathtrace.scene import Plane, Union, to_text

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# (name in tests/golden/spans_<name>.npz, builder), as tests/test_queries.py builds them
SPAN_SCENES = {"csg": "csg_zoo", "p1": "scene_p1"}
SHADE_SCENES = list(T.TEX_EVAL_SCENES) + ["scene_p1"]
# the guide frames: the closed scenes, and the CSG zoo without its sky wall (csg_open), whose frame has
# pixels that some samples hit and others miss
GUIDE_SCENES = ["scene_p1", "csg_zoo", "p1_coord", "csg_open"]


def csg_open():
    """zoo.csg_zoo() without the sky wall (the plane with normal +z) that closes it behind everything"""
    def drop(o):
        if isinstance(o, Union):
            a, b = drop(o.a), drop(o.b)
            return b if a is None else a if b is None else Union(a, b)
        return None if isinstance(o, Plane) and tuple(float(v) for v in o.normal) == (0.0, 0.0, 1.0) else o
    return drop(T.csg_zoo())


def with_coord_emitters(text):
    """the text scene with one more texture, `coord` (getColor(v) = v), as every material's emissive
    texture: the emission of a hit is then its position"""
    tid = 1 + max(int(m) for m in re.findall(r"^tex (\d+) ", text, flags=re.M))
    lines, out, done = text.splitlines(), [], False
    for ln in lines:
        f = ln.split()
        if f and f[0] == "mat":
            if not done:
                out.append("tex %d coord" % tid)
                done = True
            f[4] = str(tid)  # mat <id> <refl> <scat> <emis> ...
            ln = " ".join(f)
        out.append(ln)
    assert done
    return "\n".join(out) + "\n"


def text(name, img_dir):
    """the text of a scene builder of tests/zoo.py / pathtrace.scenes, or of "p1_coord"; image files
    go to img_dir"""
    if name == "p1_coord":
        return with_coord_emitters(to_text(T.build("scene_p1"), str(img_dir)))
    if name == "csg_open":
        return to_text(csg_open(), str(img_dir))
    return to_text(T.build(name), str(img_dir))


def seam_texts():
    """{tree name: scene text} of tests/golden/fastcheck_seam.npz"""
    with np.load(os.path.join(GOLD, "fastcheck_seam.npz")) as z:
        return {k[len("text_"):]: str(z[k]) for k in z.files if k.startswith("text_")}
