"""NumPy restatement of the reference's RGB loader (trainer.py:75-123; the same chain in pruner.py, labelPropTrain.py, tester.py,
makeLPImages.py, classTrainer.py, objDetEval.py): ``Scale`` -> ``HorizontalFlip`` -> ``VerticalFlip`` -> torchvision's PIL
``ColorJitter`` -> skimage ``rgb2yuv`` -> ``ToTensor`` -> ``Normalize([.5, 0, 0], [.5, .5, .5])``, and the label's ``Scale`` / flips /
``maskLabel``.  A helper of the tests, not a test: tests/test_rgb_prep.py pins steps 1-3 to live Pillow, tests/test_gpu_rgb_prep.py
pins the kernel (RCV_OP_RGB_PREP, ``prepare_rgb_batch``) to this file.

Pinned to Pillow (12.2.0): the resize (tests/batch_prep_restatement.py), ``Image.blend`` and the three ``ImageEnhance`` operations,
``convert("L")``, ``convert("HSV")`` and back.  The project's definition (skimage is not available to pin them): step 4, float64 with
``byte / 255.0`` and the three products of a matrix row summed left to right.

The parameter row of an image (float32 [12], ``data.draw_color_jitter``): {hflip, vflip, n_ops, op0, op1, op2, op3, f_brightness,
f_contrast, f_saturation, hue_shift, 0}; op codes 0 = brightness, 1 = contrast, 2 = saturation, 3 = hue, -1 = unused."""
import numpy as np

from batch_prep_restatement import FLAG_SETS, mask_label, resize_bilinear, resize_nearest, synthetic_frames  # noqa: F401

OP_BRIGHTNESS, OP_CONTRAST, OP_SATURATION, OP_HUE = 0, 1, 2, 3
YUV = np.array([[0.299, 0.587, 0.114], [-0.14714119, -0.28886916, 0.43601035], [0.61497538, -0.51496512, -0.10001026]], np.float64)
F32 = np.float32


def luma(rgb):
    """Pillow's convert("L") of uint8 [..., 3]: (19595 R + 38470 G + 7471 B + 32768) >> 16."""
    c = rgb.astype(np.int64)
    return ((19595 * c[..., 0] + 38470 * c[..., 1] + 7471 * c[..., 2] + 32768) >> 16).astype(np.uint8)


def blend(d, x, f):
    """Image.blend(d, x, f) per byte: t = d + f (x - d) in float32, multiply and add rounded separately; 0 if t <= 0, 255 if
    t >= 255, else t truncated."""
    f = F32(f)
    d = np.asarray(d).astype(F32)
    x = np.asarray(x).astype(F32)
    t = (d + (f * (x - d)).astype(F32)).astype(F32)
    return np.where(t <= 0, 0, np.where(t >= 255, 255, np.minimum(np.maximum(t, 0), 255).astype(np.int32))).astype(np.uint8)


def contrast_mean(rgb):
    """int(ImageStat.Stat(img.convert("L")).mean[0] + 0.5) = floor((2 sum L + n) / (2 n)) over the whole image."""
    lum = luma(rgb)
    n = lum.size
    return int((2 * int(lum.astype(np.int64).sum()) + n) // (2 * n))


def rgb_to_hsv(rgb):
    """Pillow's convert("HSV") of uint8 [..., 3]."""
    c = rgb.astype(np.int32)
    r, g, b = c[..., 0], c[..., 1], c[..., 2]
    maxc, minc = np.maximum(r, np.maximum(g, b)), np.minimum(r, np.minimum(g, b))
    gray = maxc == minc
    with np.errstate(divide="ignore", invalid="ignore"):
        cr = (maxc - minc).astype(F32)
        s = cr / maxc.astype(F32)
        rc, gc, bc = (maxc - r).astype(F32) / cr, (maxc - g).astype(F32) / cr, (maxc - b).astype(F32) / cr
        rc64, gc64, bc64 = rc.astype(np.float64), gc.astype(np.float64), bc.astype(np.float64)
        h = np.where(r == maxc, bc - gc, np.where(g == maxc, ((2.0 + rc64) - bc64).astype(F32), ((4.0 + gc64) - rc64).astype(F32))).astype(F32)
        h = np.fmod(h.astype(np.float64) / 6.0 + 1.0, 1.0).astype(F32)
        hh = np.where(gray, 0.0, h.astype(np.float64) * 255.0)
        ss = np.where(gray, 0.0, s.astype(np.float64) * 255.0)
    out = np.empty(rgb.shape, np.uint8)
    out[..., 0] = np.clip(hh.astype(np.int64), 0, 255)
    out[..., 1] = np.clip(ss.astype(np.int64), 0, 255)
    out[..., 2] = maxc
    return out


def _rnd(x):
    """C's round(): half away from zero (the arguments here are never negative)."""
    return np.clip(np.floor(x.astype(np.float64) + 0.5), 0, 255).astype(np.uint8)


def hsv_to_rgb(hsv):
    """Pillow's HSV -> RGB of uint8 [..., 3], in float32."""
    h, s, v = hsv[..., 0].astype(F32), hsv[..., 1].astype(F32), hsv[..., 2].astype(F32)
    one = F32(1.0)
    hf = (h * F32(6.0)) / F32(255.0)
    i = np.floor(hf)
    f = hf - i
    fs = s / F32(255.0)
    p = _rnd(v * (one - fs))
    q = _rnd(v * (one - fs * f))
    t = _rnd(v * (one - fs * (one - f)))
    vv = hsv[..., 2]
    k = i.astype(np.int32) % 6
    r = np.choose(k, [vv, q, p, p, t, vv])
    g = np.choose(k, [t, vv, vv, q, p, p])
    b = np.choose(k, [p, p, t, vv, vv, q])
    gray = hsv[..., 1] == 0
    out = np.empty(hsv.shape, np.uint8)
    out[..., 0] = np.where(gray, vv, r)
    out[..., 1] = np.where(gray, vv, g)
    out[..., 2] = np.where(gray, vv, b)
    return out


def hue(rgb, shift):
    hsv = rgb_to_hsv(rgb)
    hsv[..., 0] = (hsv[..., 0].astype(np.int32) + int(shift)) & 255
    return hsv_to_rgb(hsv)


def brightness(rgb, f):
    return blend(0, rgb, f)


def contrast(rgb, f):
    return blend(contrast_mean(rgb), rgb, f)


def saturation(rgb, f):
    return blend(luma(rgb)[..., None], rgb, f)


def color_ops(rgb, row):
    """Step 3: the first n_ops operations of the row, in its order, on a uint8 [H][W][3] image."""
    row = np.asarray(row, F32)
    for k in range(int(row[2])):
        op = int(row[3 + k])
        if op == OP_BRIGHTNESS:
            rgb = brightness(rgb, row[7])
        elif op == OP_CONTRAST:
            rgb = contrast(rgb, row[8])
        elif op == OP_SATURATION:
            rgb = saturation(rgb, row[9])
        elif op == OP_HUE:
            rgb = hue(rgb, int(row[10]))
    return rgb


def pillow_color_ops(rgb, row):
    """Step 3 as the Pillow calls torchvision's PIL ColorJitter makes (ImageEnhance.*.enhance, adjust_hue's HSV round trip)."""
    from PIL import Image, ImageEnhance
    row = np.asarray(row, F32)
    im = Image.fromarray(np.ascontiguousarray(rgb))
    for k in range(int(row[2])):
        op = int(row[3 + k])
        if op == OP_BRIGHTNESS:
            im = ImageEnhance.Brightness(im).enhance(float(row[7]))
        elif op == OP_CONTRAST:
            im = ImageEnhance.Contrast(im).enhance(float(row[8]))
        elif op == OP_SATURATION:
            im = ImageEnhance.Color(im).enhance(float(row[9]))
        elif op == OP_HUE:
            h, s, v = im.convert("HSV").split()
            np_h = ((np.array(h, dtype=np.int32) + int(row[10])) & 255).astype(np.uint8)
            im = Image.merge("HSV", (Image.fromarray(np_h, "L"), s, v)).convert("RGB")
    return np.asarray(im)


def pillow_image(frame, label, size, row, flags=(False, False, False, False)):
    """One image through Pillow's own calls, the host chain of the reference (row None: the validation chain; label None: a patch):
    (float32 [3][H][W], int64 [H][W] or None, uint8 [H][W][3] after step 3)."""
    from PIL import Image
    H, W = size
    im = Image.fromarray(frame)
    lab = None if label is None else Image.fromarray(label.astype(np.int32)).convert("I")
    if frame.shape[:2] != (H, W):
        im = im.resize((W, H), Image.BILINEAR)
        lab = None if lab is None else lab.resize((W, H), Image.NEAREST)
    if row is not None:
        for k, how in ((0, Image.FLIP_LEFT_RIGHT), (1, Image.FLIP_TOP_BOTTOM)):
            if row[k] != 0:
                im = im.transpose(how)
                lab = None if lab is None else lab.transpose(how)
        rgb = pillow_color_ops(np.asarray(im), row)
    else:
        rgb = np.asarray(im)
    tgt = None if lab is None else mask_label(np.asarray(lab).astype(np.int64), *flags)
    return to_yuv(rgb), tgt, np.ascontiguousarray(rgb)


def to_yuv(rgb, reciprocal=False):
    """Step 4: float64 rgb2yuv + ToTensor + Normalize([.5, 0, 0], [.5, .5, .5]) of uint8 [..., 3] -> float32 [3][...].
    reciprocal: c = byte * (1 / 255.0), the other byte-to-float form (counted against this one in tests/test_rgb_prep.py)."""
    c = rgb.astype(np.float64) * (1.0 / 255.0) if reciprocal else rgb.astype(np.float64) / 255.0
    out = []
    for k in range(3):
        v = c[..., 0] * YUV[k, 0]
        v = v + c[..., 1] * YUV[k, 1]
        v = v + c[..., 2] * YUV[k, 2]
        out.append(((v - 0.5) / 0.5 if k == 0 else v / 0.5).astype(F32))
    return np.stack(out)


def scaled_size(Hs, Ws, scale):
    """transform.py:8-19 ``Scale``: factor 1 means no resize."""
    return (Hs, Ws) if scale == 1 else (int(Hs / scale), int(Ws / scale))


def prepare_image(frame, label, size, train=False, row=None, flags=(False, False, False, False), pillow=False, bytes_out=False):
    """One image: uint8 [Hs][Ws][3] and integer [Hs][Ws] or None -> (float32 [3][H][W], int64 [H][W] or None).
    pillow: step 3 through Pillow's own calls; bytes_out: also the uint8 [H][W][3] image after step 3."""
    H, W = size
    if frame.shape[:2] != (H, W):
        frame = resize_bilinear(frame, size)
        if label is not None:
            label = resize_nearest(label, size)
    if train:
        row = np.asarray(row, F32)
        if row[0] != 0:
            frame = frame[:, ::-1]
            label = None if label is None else label[:, ::-1]
        if row[1] != 0:
            frame = frame[::-1]
            label = None if label is None else label[::-1]
        frame = (pillow_color_ops if pillow else color_ops)(np.ascontiguousarray(frame), row)
    img = to_yuv(frame)
    lab = None if label is None else mask_label(np.ascontiguousarray(label).astype(np.int64), *flags)
    if bytes_out:
        return img, lab, np.ascontiguousarray(frame)
    return img, lab


def prepare_batch(frames, labels, size, train=False, params=None, flags=(False, False, False, False), pillow=False):
    """(float32 [B][3][H][W], int64 [B][H][W] or None)."""
    outs = [prepare_image(frames[b], None if labels is None else labels[b], size, train, None if params is None else params[b], flags, pillow)
            for b in range(len(frames))]
    return np.stack([o[0] for o in outs]), None if labels is None else np.stack([o[1] for o in outs])


def make_row(ops, fb=1.0, fc=1.0, fs=1.0, shift=0, hflip=False, vflip=False):
    """A parameter row from a list of op codes and the factors."""
    row = np.zeros(12, F32)
    row[0], row[1], row[2] = float(hflip), float(vflip), len(ops)
    row[3:7] = -1
    row[3:3 + len(ops)] = ops
    row[7], row[8], row[9], row[10] = fb, fc, fs, int(shift) & 255
    return row
