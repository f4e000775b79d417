"""The host statement of the detection overlay and of the heat-map view (include/centerpoly_hip.h: cp_render_overlay,
cp_render_heatmap), written with the installed PIL and numpy alone: PIL's ImageDraw.polygon for the fill and outline
masks, PIL's built-in bitmap font for the glyphs, numpy for the dilation, the boxes, the cells and the integer
blends, and a sequential loop in which a later operation simply overwrites an earlier one.  It shares no code with
the kernels or with centerpoly_amd.utils.debugger; the tests hold the device pictures to it pixel for pixel."""
import numpy as np
from PIL import Image, ImageDraw, ImageFont

OPS = ("fill", "outline", "box", "label_bg", "glyph")
_FONT = ImageFont.load_default_imagefont()


def to_int(v):
    """The writers' vertex: int(float('%.2f' % v))."""
    return int(float("{:.2f}".format(v)))


def instances(rows, thresh, num_classes):
    """Rows [R, 2N + 7] (x1,y1,x2,y2,score,cls,poly,depth) -> the drawn instances, nearest first: ascending depth,
    ties by class and then by row.  Each: (row index, class, score, [(x, y)], (x1, y1, x2, y2))."""
    rows = np.asarray(rows, np.float32)
    live = [k for k in range(len(rows))
            if rows[k, 4] > np.float32(thresh) and 0 <= rows[k, 5] < num_classes and rows[k, 5] == int(rows[k, 5])]
    live.sort(key=lambda k: (float(rows[k, -1]), int(rows[k, 5]), k))
    out = []
    for k in live:
        poly = [to_int(v) for v in rows[k, 6:-1]]
        box = tuple(int(np.trunc(np.clip(np.float64(v), -2147483648.0, 2147483520.0))) for v in rows[k, :4])
        out.append((k, int(rows[k, 5]), rows[k, 4], list(zip(poly[0::2], poly[1::2])), box))
    return out


def fill_mask(pts, W, H):
    im = Image.new("L", (W, H), 0)
    ImageDraw.Draw(im).polygon(pts, fill=255)
    return np.asarray(im) != 0


def outline_mask(pts, W, H):
    im = Image.new("L", (W, H), 0)
    ImageDraw.Draw(im).polygon(pts, outline=255)
    return np.asarray(im) != 0


def dilate(mask, r):
    """By the (2r + 1) x (2r + 1) square, clipped to the canvas."""
    H, W = mask.shape
    pad = np.zeros((H + 2 * r, W + 2 * r), bool)
    pad[r:r + H, r:r + W] = mask
    out = np.zeros((H, W), bool)
    for dy in range(2 * r + 1):
        for dx in range(2 * r + 1):
            out |= pad[dy:dy + H, dx:dx + W]
    return out


def glyph(ch):
    """bool [11, 6]: the character drawn alone at (0, 0) of its cell; outside chr(32) .. chr(127) a blank cell."""
    if not 32 <= ord(ch) <= 127:
        return np.zeros((11, 6), bool)
    cell = Image.new("L", (6, 11), 0)
    ImageDraw.Draw(cell).text((0, 0), ch, fill=255, font=_FONT)
    return np.asarray(cell) != 0


def label(name, score):
    return ("%s%.1f" % (name, float(score)))[:16]


def overlay(image, rows, thresh, names, palette, white=False, show_txt=True, alpha=102, r=1, t=2,
            outline=(0, 255, 255), show_polygons=True):
    """-> (picture uint8 [H, W, 3], winner uint8 [H, W]: 0 untouched, else 1 + index into OPS of the operation
    shown).  palette: uint8 [C, 3] in the image's channel order."""
    image = np.asarray(image, np.uint8)
    H, W = image.shape[:2]
    inst = instances(rows, thresh, len(names))
    if len(inst) > 128:
        raise ValueError("more than 128 instances in one image (max_per_image = K <= 128)")
    canvas, winner = image.copy(), np.zeros((H, W), np.uint8)
    yy, xx = np.arange(H, dtype=np.int64)[:, None], np.arange(W, dtype=np.int64)[None, :]
    for _, cls, score, pts, (x1, y1, x2, y2) in reversed(inst):           # farthest first
        colour = np.asarray(palette[cls], np.int64)
        if white:
            colour = 255 - colour
        if show_polygons and max(abs(v) for pt in pts for v in pt) <= 1 << 29:   # farther out: no defined drawing
            F = fill_mask(pts, W, H)
            canvas[F] = ((image[F].astype(np.int64) * (256 - alpha) + colour * alpha + 128) >> 8).astype(np.uint8)
            winner[F] = 1
            O = dilate(outline_mask(pts, W, H), r)
            canvas[O] = np.asarray(outline, np.uint8)
            winner[O] = 2
        inside = (xx >= x1) & (xx <= x2) & (yy >= y1) & (yy <= y2)
        near = np.minimum(np.minimum(xx - x1, x2 - xx), np.minimum(yy - y1, y2 - yy)) < t
        B = inside & near
        canvas[B] = colour.astype(np.uint8)
        winner[B] = 3
        if show_txt:
            text = label(names[cls], score)
            G = (xx >= x1) & (xx < x1 + 6 * len(text)) & (yy >= y1 - 12) & (yy <= y1 - 2)
            canvas[G] = colour.astype(np.uint8)
            winner[G] = 4
            for j, ch in enumerate(text):
                for cy, cx in zip(*np.nonzero(glyph(ch))):
                    x, y = x1 + 6 * j + int(cx), y1 - 12 + int(cy)
                    if 0 <= x < W and 0 <= y < H:
                        canvas[y, x] = 0
                        winner[y, x] = 5
    return canvas, winner


def check_condition(image, picture, winner, show_txt=True):
    """The condition every drawn case must meet on the host statement alone: at least 1 % of the pixels differ
    from the input and every operation kind wins at least one pixel (four kinds without text)."""
    changed = (picture != image).any(axis=2).mean()
    assert changed >= 0.01, "only %.3f %% of the pixels changed" % (100 * changed)
    for k in range(1, 6 if show_txt else 4):
        assert (winner == k).any(), "operation %s wins no pixel" % OPS[k - 1]
    if not show_txt:
        assert not (winner >= 4).any()


def heatmap(hm, net_input, mean, std, palette, ratio, white=False):
    """hm float32 [C, h, w] (activated), net_input float32 [3, h ratio, w ratio] -> uint8 [h ratio, w ratio, 3]."""
    hm, net_input = np.asarray(hm, np.float32), np.asarray(net_input, np.float32)
    palette = np.asarray(palette, np.uint8)
    C, h, w = hm.shape
    cm = np.zeros((h, w, 3), np.uint8)
    for c in range(C):
        col = palette[c % len(palette)].astype(np.float32)
        cm = np.maximum(cm, (hm[c][:, :, None] * col[None, None, :]).astype(np.uint8))
    cm = cm.repeat(ratio, axis=0).repeat(ratio, axis=1)
    if white:
        cm = 255 - cm
    mean, std = np.asarray(mean, np.float32).reshape(1, 1, 3), np.asarray(std, np.float32).reshape(1, 1, 3)
    back = (net_input.transpose(1, 2, 0) * std + mean) * np.float32(255)
    back = np.clip(back, 0, 255).astype(np.uint8)
    return ((back.astype(np.int64) * 77 + cm.astype(np.int64) * 179 + 128) >> 8).astype(np.uint8)
