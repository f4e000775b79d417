"""Generates tests/golden/ground_truth.npz: what the evaluators' preparation scripts draw for the inputs of
ground_truth_cases.py.  Run from the repository root where the reference lies beside it:
    python tests/golden/gen_ground_truth_golden.py [REFERENCE_ROOT]

The reference's own `createInstanceImage` and `createLabelImage` run here, for IDD
(src/lib/datasets/evaluation/IDDscripts/preperation/json2instanceImg.py, json2labelImg.py) and for Cityscapes
(.../cityscapesscripts/preparation/...), on `Annotation` objects read from the cases' JSON text, with the installed
PIL.  The scripts are loaded from their files as they are.  What they miss here is supplied from outside: PIL 12 has no
`PILLOW_VERSION` (an attribute is set before they load), and the IDD label script calls `tqdm.write` without importing
tqdm (the name is put into its module).  To record WHAT is drawn, each script's `ImageDraw` name is replaced by a
recorder that notes (fill, vertices) of every `polygon` call and hands the call on to PIL's drawer.

The fixture holds, per case, the drawn sequence (values, vertex counts, vertices truncated towards zero as PIL takes
them) and the image; per driver frame the default images of both kinds; and the two label tables as arrays."""
import importlib.util
import json
import os
import sys
import types

import numpy as np
import PIL
from PIL import ImageDraw

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import ground_truth_cases as gc  # noqa: E402

EVAL = "src/lib/datasets/evaluation"


def load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class Recorder(object):
    """Stands where a script expects the ImageDraw module."""

    def __init__(self):
        self.log = []

    def Draw(self, image):
        real, log = ImageDraw.Draw(image), self.log

        def polygon(xy, fill=None, outline=None):
            assert outline is None
            log.append((fill, [(p[0], p[1]) for p in xy]))
            real.polygon(xy, fill=fill)
        return types.SimpleNamespace(polygon=polygon)


def reference_scripts(ref):
    """{(dataset, kind): (function(annotation, encoding) -> PIL image, Annotation class, recorder)}."""
    if not hasattr(PIL, "PILLOW_VERSION"):
        PIL.PILLOW_VERSION = PIL.__version__
    base = os.path.join(ref, EVAL)
    sys.path.insert(0, base)                                          # cityscapesscripts.helpers...
    sys.path.insert(0, os.path.join(base, "IDDscripts", "helpers"))   # anue_labels, annotation
    import tqdm
    out, tables = {}, {}
    prep = os.path.join(base, "IDDscripts", "preperation")
    inst = load("ref_idd_json2instanceImg", os.path.join(prep, "json2instanceImg.py"))
    lab = load("ref_idd_json2labelImg", os.path.join(prep, "json2labelImg.py"))
    lab.tqdm = tqdm.tqdm
    for kind, mod, fn in (("instance", inst, "createInstanceImage"), ("label", lab, "createLabelImage")):
        rec = Recorder()
        mod.ImageDraw = rec
        out[("IDD", kind)] = (lambda a, e, f=getattr(mod, fn): f("case.json", a, e), mod.Annotation, rec)
    tables["IDD"] = inst.labels
    prep = os.path.join(base, "cityscapesscripts", "preparation")
    inst = load("ref_cs_json2instanceImg", os.path.join(prep, "json2instanceImg.py"))
    lab = load("ref_cs_json2labelImg", os.path.join(prep, "json2labelImg.py"))
    for kind, mod, fn in (("instance", inst, "createInstanceImage"), ("label", lab, "createLabelImage")):
        rec = Recorder()
        mod.ImageDraw = rec
        out[("cityscapes", kind)] = (lambda a, e, f=getattr(mod, fn): f(a, e), mod.Annotation, rec)
    tables["cityscapes"] = inst.labels
    return out, tables


def draw(scripts, dataset, kind, encoding, frame):
    """(values int32 [m], counts int32 [m], xy int32 [T, 2], image int32 [H, W]) of one polygon file."""
    fn, Annotation, rec = scripts[(dataset, kind)]
    a = Annotation()
    a.fromJsonText(json.dumps(frame))
    del rec.log[:]
    img = np.array(fn(a, encoding)).astype(np.int32)
    assert img.shape == (frame["imgHeight"], frame["imgWidth"])
    values = np.array([v for v, _ in rec.log], np.int32)
    counts = np.array([len(p) for _, p in rec.log], np.int32)
    pts = [np.trunc(np.asarray(p, np.float64)).astype(np.int32).reshape(-1, 2) for _, p in rec.log]
    xy = np.concatenate(pts) if pts else np.zeros((0, 2), np.int32)
    return values, counts, xy, img


def main(ref):
    scripts, tables = reference_scripts(ref)
    out = {}
    for name, (dataset, kind, encoding, canvas, build) in sorted(gc.CASES.items()):
        values, counts, xy, img = draw(scripts, dataset, kind, encoding, gc.frame_json(name))
        out["%s_values" % name], out["%s_counts" % name], out["%s_xy" % name] = values, counts, xy
        out["%s_image" % name] = img
    defaults = {"IDD": "id", "cityscapes": "ids"}
    for dataset, frames in (("IDD", gc.IDD_FRAMES), ("cityscapes", gc.CITYSCAPES_FRAMES)):
        for city, stem, case in frames:
            for kind in ("instance", "label"):
                out["frame_%s_%s_%s" % (dataset, case, kind)] = draw(scripts, dataset, kind, defaults[dataset],
                                                                     gc.frame_json(case))[3]
    # the label tables: names, the ids of every encoding in the scripts' order, has instances
    t = tables["IDD"]
    out["table_IDD_names"] = np.array([l.name for l in t], dtype="U32")
    out["table_IDD_ids"] = np.array([[l.id, l.csId, l.csTrainId, l.level4Id, l.level3Id, l.level2Id, l.level1Id]
                                     for l in t], np.int32)
    out["table_IDD_instances"] = np.array([l.hasInstances for l in t], bool)
    t = tables["cityscapes"]
    out["table_cityscapes_names"] = np.array([l.name for l in t], dtype="U32")
    out["table_cityscapes_ids"] = np.array([[l.id, l.trainId] for l in t], np.int32)
    out["table_cityscapes_instances"] = np.array([l.hasInstances for l in t], bool)

    dst = os.path.join(HERE, "ground_truth.npz")
    np.savez_compressed(dst, **out)
    print("wrote %s: %d arrays, %d bytes" % (dst, len(out), os.path.getsize(dst)))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(ROOT), "reference"))
