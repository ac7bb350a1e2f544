"""robocupvision_amd: the ROBO-UNet / U-Net training hot path of szemenyeim/RoboCupVision as
hand-written HIP kernels for MI355X (gfx950), behind the reference's nn.Module surface.

    from robocupvision_amd.model import ROBO_UNet, CrossEntropyLoss2d      # drop-in for `from model import *`
"""
__version__ = "0.1.0"


def __getattr__(name):
    # robocupvision_amd.labelprop_batch(images, labels): the batch assembly of labelPropTrain.py (model.py); imported on first use so
    # that `import robocupvision_amd` stays free of torch
    if name == "labelprop_batch":
        from .model import labelprop_batch
        return labelprop_batch
    # ... and robocupvision_amd.labelprop_next(cur, prev, prior): the same input from a prediction of the previous frame
    if name == "labelprop_next":
        from .model import labelprop_next
        return labelprop_next
    # the FCN of the reference's shipped segmentation checkpoints, its blocks and the separable blocks (model.py:84-90, 144-164, 235-254, 311-377)
    if name in ("FCN", "DownSamplerThick", "ConvPoolDouble", "View", "ConvSep", "trConvSep"):
        from . import model
        return getattr(model, name)
    # robocupvision_amd.data / prepare_batch / draw_jitter / SSYUVDataset: batches prepared on the device (data.py)
    if name == "data":
        import importlib
        return importlib.import_module(".data", __name__)
    # ... and the RGB loader of trainer.py / pruner.py: prepare_rgb_batch / draw_color_jitter / SSDataSet
    if name in ("prepare_batch", "prepare_frames", "draw_jitter", "SSYUVDataset", "prepare_rgb_batch", "draw_color_jitter", "SSDataSet"):
        from . import data
        return getattr(data, name)
    # ... and whole epochs from a dataset that stays on the device as resized bytes: resize_u8 / ResidentDataset / EpochLoader
    if name in ("resize_u8", "draw_jitter_rows", "ResidentDataset", "EpochLoader"):
        from . import data
        return getattr(data, name)
    # ... the RGB loader's epochs and LabelProp's frame pairs from the same store: RGBEpochLoader / LPDataSet / LPEpochLoader
    if name in ("prepare_lp_pairs", "draw_color_jitter_rows", "RGBEpochLoader", "LPDataSet", "LPEpochLoader"):
        from . import data
        return getattr(data, name)
    # class maps and colour masks on the device (detect.py): palette.py, infer.py
    if name in ("colorize", "Colorize", "labelcolormap"):
        from . import palette
        return getattr(palette, name)
    # ... and the objects of a class map (test.py:43-67, DBConvert.py:47-102): find_objects
    if name in ("Segmenter", "find_objects", "Objects", "DBCONVERT", "LabelPropagator"):
        from . import infer
        return getattr(infer, name)
    # ... and the cleaning between the two (labelExtraction.py:70-89 __filterMask; test.py:41's commented MORPH_CLOSE): RCV_OP_MAP_FILTER
    if name in ("majority_filter", "erode_map", "open_map", "close_map", "trim_pseudo_labels"):
        from . import infer
        return getattr(infer, name)
    # ... and the patches of those objects, cut out of the full-resolution frames for the patch classifiers: patches.py
    if name == "patches":
        import importlib
        return importlib.import_module(".patches", __name__)
    if name in ("object_patches", "classify_objects", "classify_patches", "Patches"):
        from . import patches
        return getattr(patches, name)
    # label propagation by dense optical flow (test.py:135-140 --lProp; transform.py:185-198): flow.py
    if name == "flow":
        import importlib
        return importlib.import_module(".flow", __name__)
    if name in ("farneback_flow", "update_labels", "propagate_labels", "rgb_to_gray", "optFlow", "updateLabels"):
        from . import flow
        return getattr(flow, name)
    # the robot-side export (net.cfg + weights.dat), written and read back: export.py
    if name in ("net_cfg", "save_export", "load_export", "ExportedNet", "saveParams", "loadParams"):
        from . import export
        return getattr(export, name)
    raise AttributeError("module %r has no attribute %r" % (__name__, name))
