"""Fixtures of the robot-side export tests (tests/test_export_load.py, tests/test_gpu_export.py).  Runs ONLY where the reference
checkout exists (REF below); it imports the reference's ``model.py`` at generation time, as make_golden.py does, and stores data and
settings only:

  export_lp/net.cfg, export_lp/weights.dat   the LabelProp export the reference ships (weightsLP/): the layer-settings file and the
                                             92 837 float64 values of pth/bestModelLPFinetunedPruned.pth in state_dict order without
                                             num_batches_tracked (asserted here, element for element)
  export_vga.cfg                             the layer-settings file of weightsVGA/ (PB_FCN(32, 5, 1, True, 0) at 480 x 640)
  export_lp.npz                              x_<tag>: inputs by the labelPropTrain.py:178-182 recipe (labels constant on 8 x 8
                                             blocks) at 2 x 8 x 40 x 56 and 2 x 8 x 24 x 32; logits_<tag>: the reference's output for
                                             them with the pruned checkpoint; proba_<tag> / argmax_<tag>: their float64 softmax and
                                             arg-max

A seed is accepted when at most 0.1 % of the pixels have a top-2 logit gap below 1e-4 (the class map is judged outside them)."""
import os
import shutil
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
SHAPES = {"40x56": (40, 56), "24x32": (24, 32)}
NEAR, NEAR_SHARE = 1e-4, 1e-3


def reference_labelprop(ref):
    """ref.LabelProp(5, 32, 0.0) with the pruned checkpoint.  The class cannot be constructed at HEAD (8 arguments passed to a 7-argument
    ConvPoolSimple.__init__): the constructor is wrapped to drop the extra (dropout) argument, as make_golden.py does."""
    orig = ref.ConvPoolSimple.__init__

    def patched(self, inplanes, planes, size, stride, padding, dilation, bias, *_ignored):
        orig(self, inplanes, planes, size, stride, padding, dilation, bias)
    ref.ConvPoolSimple.__init__ = patched
    try:
        net = ref.LabelProp(5, 32, 0.0)
    finally:
        ref.ConvPoolSimple.__init__ = orig
    net.load_state_dict(torch.load(os.path.join(REF, "pth", "bestModelLPFinetunedPruned.pth"), map_location="cpu"))
    return net.eval()


def inputs(H, W, seed):
    sys.path.insert(0, os.path.join(HERE, "..", ".."))
    from oracle.cpu_reference import labelprop_inputs
    g = torch.Generator().manual_seed(seed)
    y_t = torch.randn(H, W, generator=g)
    y_n = y_t + 0.1 * torch.randn(H, W, generator=g)
    blocks = lambda: torch.randint(0, 5, (H // 8, W // 8), generator=g).repeat_interleave(8, 0).repeat_interleave(8, 1)
    return labelprop_inputs(y_t, y_n, blocks(), blocks())


def main():
    sys.path.insert(0, REF)
    import model as ref          # the reference, imported (never copied)
    os.makedirs(os.path.join(HERE, "export_lp"), exist_ok=True)
    for src, dst in ((("weightsLP", "net.cfg"), ("export_lp", "net.cfg")), (("weightsLP", "weights.dat"), ("export_lp", "weights.dat")),
                     (("weightsVGA", "net.cfg"), ("export_vga.cfg",))):
        shutil.copyfile(os.path.join(REF, *src), os.path.join(HERE, *dst))
        os.chmod(os.path.join(HERE, *dst), 0o644)
    net = reference_labelprop(ref)
    flat = np.concatenate([v.numpy().reshape(-1).astype(np.float64) for k, v in net.state_dict().items() if not k.endswith("num_batches_tracked")])
    dat = np.fromfile(os.path.join(HERE, "export_lp", "weights.dat"), dtype=np.float64)
    assert dat.size == 92837 and np.array_equal(dat, flat), "weightsLP/weights.dat is not the pruned checkpoint in state_dict order"
    print("weights.dat: %d values, %.1f %% zeros" % (dat.size, 100.0 * float((dat == 0).mean())))
    out = {}
    for tag, (H, W) in SHAPES.items():
        for seed in range(40, 60):
            x = inputs(H, W, seed)
            with torch.no_grad():
                y = net(x.clone())
            top2 = torch.topk(y, 2, dim=1)[0]
            share = float(((top2[:, 0] - top2[:, 1]) < NEAR).double().mean())
            if share <= NEAR_SHARE:
                break
        else:
            raise AssertionError("no seed with at most %.1f %% near-tie pixels at %s" % (100 * NEAR_SHARE, tag))
        p = torch.softmax(y.double(), 1)
        conf = p.max(1)[0]
        print("%s: seed %d, near ties %.3f %%, classes %s, confidence < 0.9 on %.1f %% of the pixels"
              % (tag, seed, 100 * share, sorted(set(torch.max(y, 1)[1].reshape(-1).tolist())), 100 * float((conf < 0.9).double().mean())))
        out["x_" + tag] = x.numpy()
        out["logits_" + tag] = y.numpy()
        out["proba_" + tag] = p.numpy()
        out["argmax_" + tag] = torch.max(y, 1)[1].numpy().astype(np.uint8)
    np.savez_compressed(os.path.join(HERE, "export_lp.npz"), **out)


if __name__ == "__main__":
    main()
