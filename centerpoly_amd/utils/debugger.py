"""Debugger (reference: src/lib/utils/debugger.py), headless and on the device.

The reference draws with cv2 on host arrays and shows windows.  Here the pictures are device uint8 tensors composed
by HIP kernels (csrc/render.hip): `add_polydet_detections` runs cp_writer_instances + cp_render_overlay on the
detection rows that post_process left on the device, `add_blend_img` runs cp_render_heatmap.  The host builds the
small tables (palette, glyph atlas, label codes) and encodes PNG files; `show_all_imgs` writes files because there is
no display.  No pixel parity with cv2's drawing is claimed: the picture is defined in include/centerpoly_hip.h in
terms PIL and numpy reproduce exactly (tests/golden/render_host.py).

Channel order: pictures are in the caller's order, BGR in the drivers (cv2.imread's layout); palette and outline
colour are stored in that order, and the PNG writer swaps to RGB."""
import colorsys
import ctypes
import os

import numpy as np

MAX_INSTANCES = 128
MAX_LABEL = 16
CELL_W, CELL_H = 6, 11
FIRST_GLYPH, NUM_GLYPHS = 32, 96                             # the atlas holds chr(32) .. chr(127)
FILL_ALPHA = 102                                             # of 256: the class colour's weight in the fill
OUTLINE_RADIUS = 1
BOX_THICKNESS = 2
OUTLINE_RGB = (255, 255, 0)                                  # (0, 255, 255) in BGR order


def palette_rgb(num_classes):
    """uint8 [C, 3] RGB: a hue walk by the golden ratio at constant saturation and value, so neighbouring classes
    get far-apart hues.  A pure function of the class index."""
    out = np.zeros((num_classes, 3), np.uint8)
    for c in range(num_classes):
        r, g, b = colorsys.hsv_to_rgb((0.07 + c * 0.6180339887498949) % 1.0, 0.85, 0.95)
        out[c] = [int(round(255 * r)), int(round(255 * g)), int(round(255 * b))]
    return out


def glyph_atlas():
    """uint8 [96, 11, 6]: chr(32 + g) of PIL's built-in bitmap font, drawn alone at (0, 0) of a 6 x 11 cell,
    1 = set pixel."""
    from PIL import Image, ImageDraw, ImageFont
    font = ImageFont.load_default_imagefont()
    atlas = np.zeros((NUM_GLYPHS, CELL_H, CELL_W), np.uint8)
    for g in range(NUM_GLYPHS):
        cell = Image.new("L", (CELL_W, CELL_H), 0)
        ImageDraw.Draw(cell).text((0, 0), chr(FIRST_GLYPH + g), fill=255, font=font)
        atlas[g] = np.asarray(cell) != 0
    return atlas


def label_text(name, score):
    """The reference's `name + '{:.1f}'.format(score)`, cut to 16 characters."""
    return ("%s%.1f" % (name, float(score)))[:MAX_LABEL]


def label_codes(text):
    """int32 [16]: the glyph code of every character (a character outside the atlas is the blank cell of the
    space), -1 behind the end."""
    codes = np.full((MAX_LABEL,), -1, np.int32)
    for k, ch in enumerate(text[:MAX_LABEL]):
        o = ord(ch) - FIRST_GLYPH
        codes[k] = o if 0 <= o < NUM_GLYPHS else 0
    return codes


class Debugger(object):
    def __init__(self, class_names, theme="black", down_ratio=4, device=None):
        """class_names: the data set's class_name without the background entry."""
        import torch
        if theme not in ("white", "black"):
            raise ValueError("debugger theme must be white or black, got %r" % (theme,))
        self.names = list(class_names)
        self.num_classes = len(self.names)
        self.white = theme == "white"
        self.down_ratio = down_ratio
        self.device = device or torch.device("cuda")
        self.imgs = {}                                       # img_id -> device uint8 [H, W, 3]
        self.last_n = 0
        self.palette_bgr = np.ascontiguousarray(palette_rgb(self.num_classes)[:, ::-1])
        self._palette = self._atlas = None                   # device copies, made once

    def _tables(self):
        import torch
        if self._palette is None:
            self._palette = torch.from_numpy(self.palette_bgr).to(self.device)
            self._atlas = torch.from_numpy(glyph_atlas()).to(self.device)
        return self._palette, self._atlas

    # ------------------------------------------------------------------------------------------ pictures --
    def add_img(self, img, img_id="default"):
        """img: 8-bit [H, W, 3], a host array or a device tensor (copied either way)."""
        import torch
        if torch.is_tensor(img):
            t = img.to(self.device).clone()
        else:
            t = torch.from_numpy(np.ascontiguousarray(img)).to(self.device)
        if t.dtype != torch.uint8 or t.dim() != 3 or t.shape[2] != 3:
            raise TypeError("add_img needs an 8-bit [H,W,3] image (got %s %s)" % (t.dtype, tuple(t.shape)))
        self.imgs[img_id] = t.contiguous()

    def add_blend_img(self, net_input, hm, mean, std, img_id="blend"):
        """The heat-map view: gen_colormap(hm) blended over the de-normalised network input.  net_input: device
        float32 [3, H, W]; hm: device float32 [C, H / down_ratio, W / down_ratio], activated, or None for the
        de-normalised input alone."""
        import torch

        from .. import _C
        palette, _ = self._tables()
        net_input = net_input.contiguous()
        ratio = self.down_ratio
        if hm is None:
            C, h, w = 0, int(net_input.shape[1]) // ratio, int(net_input.shape[2]) // ratio
        else:
            hm = hm.contiguous()
            C, h, w = (int(v) for v in hm.shape)
        if tuple(net_input.shape) != (3, h * ratio, w * ratio):
            raise ValueError("input %s does not match the heat map %s x %d" % (tuple(net_input.shape), (h, w), ratio))
        out = torch.empty((h * ratio, w * ratio, 3), dtype=torch.uint8, device=net_input.device)
        m = np.ascontiguousarray(np.asarray(mean, np.float32).reshape(3))
        s = np.ascontiguousarray(np.asarray(std, np.float32).reshape(3))
        _C.check(_C.lib().cp_render_heatmap(_C.ptr(hm), C, h, w, ratio, _C.ptr(net_input),
                                            m.ctypes.data_as(ctypes.c_void_p), s.ctypes.data_as(ctypes.c_void_p),
                                            _C.ptr(palette), self.num_classes, int(self.white), _C.ptr(out),
                                            _C.stream()), "cp_render_heatmap")
        self.imgs[img_id] = out
        return out

    def row_labels(self, host_rows):
        """int32 [R, 16] glyph codes, one label per source row [.., score at 4, class at 5, ..]."""
        codes = np.full((len(host_rows), MAX_LABEL), -1, np.int32)
        for k, row in enumerate(host_rows):
            c = int(row[5])
            if 0 <= c < self.num_classes:
                codes[k] = label_codes(label_text(self.names[c], row[4]))
        return codes

    def add_polydet_detections(self, rows_dev, host_rows, thresh, img_id="default", show_txt=True, boxes_only=False,
                               alpha=FILL_ALPHA, radius=OUTLINE_RADIUS, thickness=BOX_THICKNESS):
        """Draws, in place on picture img_id, the detections of device rows [R, 2N + 7] (x1,y1,x2,y2,score,cls,
        poly,depth) with score > thresh.  host_rows: the same rows on the host (post_process copied them back
        already), read for the labels only; None with show_txt=False.  boxes_only hides fill and outline (the
        reference's out_pred view draws boxes alone)."""
        import torch

        from .. import _C
        img = self.imgs[img_id]
        H, W = int(img.shape[0]), int(img.shape[1])
        if rows_dev.dim() != 2 or rows_dev.dtype != torch.float32 or rows_dev.shape[1] < 13 or rows_dev.shape[1] % 2 == 0:
            raise ValueError("rows must be float32 [R, 2N + 7], got %s %s" % (rows_dev.dtype, tuple(rows_dev.shape)))
        R, N = int(rows_dev.shape[0]), (int(rows_dev.shape[1]) - 7) // 2
        if R == 0:
            self.last_n = 0
            return img
        rows_dev = rows_dev.contiguous()
        dev = rows_dev.device
        palette, atlas = self._tables()
        L = _C.lib()
        table = np.ascontiguousarray(np.stack([np.arange(self.num_classes), np.ones(self.num_classes)], 1), np.int32)
        ints = torch.empty((1 + 2 * R + (R + 3) // 4,), dtype=torch.int32, device=dev)   # n, src, label, flags
        conf = torch.empty((R,), dtype=torch.float32, device=dev)
        poly = torch.empty((R, N, 2), dtype=torch.int32, device=dev)
        at = lambda o: ctypes.c_void_p(ints.data_ptr() + 4 * o)           # noqa: E731
        st = _C.stream()
        _C.check(L.cp_writer_instances(_C.ptr(rows_dev), R, N, float(thresh), table.ctypes.data_as(ctypes.c_void_p),
                                       self.num_classes, at(0), at(1), _C.ptr(poly), at(1 + 2 * R), at(1 + R),
                                       _C.ptr(conf), st), "cp_writer_instances")
        codes = None
        if show_txt:
            codes = torch.from_numpy(self.row_labels(host_rows)).to(dev)
        params = _C.OverlayParams(int(alpha), int(radius), int(thickness), int(self.white), int(bool(show_txt)),
                                  int(not boxes_only))
        params.outline_colour[:] = OUTLINE_RGB[::-1]
        nbytes = L.cp_render_overlay_workspace_bytes(H, W)
        ws = _C.workspace(nbytes, dev)
        _C.check(L.cp_render_overlay(_C.ptr(img), H, W, _C.ptr(rows_dev), R, N, at(0), at(1), _C.ptr(poly),
                                     _C.ptr(palette), self.num_classes, _C.ptr(codes), MAX_LABEL if show_txt else 0,
                                     _C.ptr(atlas), NUM_GLYPHS, ctypes.byref(params), _C.ptr(img), _C.ptr(ws), nbytes,
                                     st), "cp_render_overlay")
        self.last_n = n = int(ints[0].item())                # read behind the picture, not before it
        if n > MAX_INSTANCES:
            raise ValueError("more than 128 instances in one image (max_per_image = K <= 128)")
        return img

    # --------------------------------------------------------------------------------------------- files --
    def save_img(self, img_id="default", path="./cache/debug/", prefix=""):
        from PIL import Image
        os.makedirs(path, exist_ok=True)
        name = os.path.join(path, "%s%s.png" % (prefix, img_id))
        bgr = self.imgs[img_id].cpu().numpy()
        Image.fromarray(np.ascontiguousarray(bgr[:, :, ::-1])).save(name)
        return name

    def save_all_imgs(self, path="./cache/debug/", prefix=""):
        return [self.save_img(img_id, path, prefix) for img_id in self.imgs]

    def show_all_imgs(self, pause=False, path="./cache/debug/", prefix=""):
        """There is no display: the pictures are written as PNG files."""
        return self.save_all_imgs(path, prefix)
