"""Float64 restatement of the validation pass (RCV_OP_CLS_VALID's counts, RCV_OP_VALID_FOLD, ``metrics.ValidationState.compute``):
valid() of train.py:97-178 from class maps, labels and the batch losses.  NumPy and plain Python only.

The state is the 76 doubles the fold keeps: [0] sum of the (fp32) batch losses, [1] batches, [2] images, [3] pixels, [4:12] iou_sum,
[12:76] conf[pred][label] in rows of 8.  ``iou_sum`` is added image by image in a sequential Python loop, in the order the device's
one-thread-per-class loop adds it, so the two can be compared bit for bit; everything else is an integer held exactly in a double.

``variant`` names a wrong reading of the source, for the tests that show the restatement tells them apart:
  "iou_summed"      IoU taken once from the batch's summed matrix instead of per image (train.py:142-153 loops over imgInd);
  "acc_in_range"    pixel accuracy over the pixels inside the confusion matrix (train.py:129 multiplies by outSize = 1 / (H * W));
  "union0_zero"     an image without the class in either mask adds 0 (train.py:150-151 adds 1)."""
import numpy as np

STATE = 76


def counts(pred, target, C):
    """int64 [N][C][C]: per image the number of pixels with (pred, label), pred < C and 0 <= label < C decided on the int64 label
    (train.py:136-147: `maskPred[c] = predClass == c`, `maskTarget[c] = targets == c`, their intersections)."""
    pred, target = np.asarray(pred).astype(np.int64), np.asarray(target).astype(np.int64)
    N = pred.shape[0]
    out = np.zeros((N, C, C), np.int64)
    for n in range(N):
        for p in range(C):
            mp = pred[n] == p
            for l in range(C):
                out[n, p, l] = int(np.sum(mp & (target[n] == l)))
    return out


def new_state():
    return np.zeros(STATE, np.float64)


def fold(state, cnt, loss, H, W, variant=None):
    """One batch into the state (a new array): cnt int [N][C][C], loss = the batch's fp32 loss value."""
    cnt = np.asarray(cnt).astype(np.int64)
    N, C, _ = cnt.shape
    s = np.array(state, np.float64)
    s[0] += float(np.float32(loss))                    # train.py:131 losstotal += loss.item()
    s[1] += 1.0
    s[2] += float(N)
    s[3] += float(N * H * W)
    for c in range(C):
        acc = float(s[4 + c])
        if variant == "iou_summed":
            tot = cnt.sum(0)
            inter = int(tot[c, c])
            union = int(tot[c, :].sum()) + int(tot[:, c].sum()) - inter
            acc += N * (1.0 if union == 0 else inter / union)
        else:
            for n in range(N):                         # train.py:142-153, image order
                inter = int(cnt[n, c, c])
                union = int(cnt[n, c, :].sum()) + int(cnt[n, :, c].sum()) - inter
                if union == 0:
                    acc += 0.0 if variant == "union0_zero" else 1.0
                else:
                    acc += inter / union
        s[4 + c] = acc
    tot = cnt.sum(0)
    for p in range(C):
        for l in range(C):
            s[12 + 8 * p + l] += float(tot[p, l])
    return s


def report(state, C, variant=None):
    """train.py:157-164 in float64; 0 / 0 is NaN, as the reference's tensors divide."""
    s = np.asarray(state, np.float64)
    conf = np.array([[s[12 + 8 * p + l] for l in range(C)] for p in range(C)], np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        lab_cnt = conf.sum(0)
        percent = conf / (lab_cnt / 100.0)[None, :]
        mean_class_acc = np.float64(0.0)
        for j in range(C):
            mean_class_acc = mean_class_acc + percent[j, j] / C
        iou = np.float64(0.0)
        for c in range(C):
            iou = iou + s[4 + c] / s[2]
        mean_iou = iou / C * 100
        trace = np.float64(sum(conf[j, j] for j in range(C)))
        pixels = conf.sum() if variant == "acc_in_range" else s[3]
        out = {"loss": float(s[0] / s[1]), "pixel_acc": float(100.0 * trace / pixels), "mean_class_acc": float(mean_class_acc),
               "mean_iou": float(mean_iou), "score": float((mean_class_acc + mean_iou) / 2), "confusion": conf.astype(np.int64),
               "confusion_percent": percent, "images": int(s[2]), "batches": int(s[1])}
    return out


def valid_pass(batches, C, variant=None):
    """batches: iterable of (pred [N,H,W], target [N,H,W], fp32 loss) -> (state, report)."""
    s = new_state()
    for pred, target, loss in batches:
        pred = np.asarray(pred)
        s = fold(s, counts(pred, target, C), loss, pred.shape[1], pred.shape[2], variant)
    return s, report(s, C, variant)
