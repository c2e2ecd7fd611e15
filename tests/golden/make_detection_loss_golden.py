#!/usr/bin/env python3
"""Pins fots_e2e.train.detection_loss to the reference's OWN loss function.

Runs in the authoring container only (needs /root/reference): imports the reference's `tools/models.py` in place and calls
`ModelResNetSep2.loss` unbound on a stub object that carries what the function reads from `self` (`angle_loss =
nn.MSELoss()`, `multi_scale`).  The function moves its two accumulators with `.cuda()`; `torch.Tensor.cuda` is patched to a
clone for the run, so that it evaluates on the CPU (a plain identity would make its in-place add hit a leaf tensor).  Stores
`detection_loss.npz`: for a handful of the small seeded cases of tests/detection_loss_cases.py, in float32, the inputs, the
three terms and the total the reference computes, and the six autograd gradients of the total.  Only arrays are stored; no
reference source travels.
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
import detection_loss_cases as DC  # noqa: E402

spec = importlib.util.spec_from_file_location("ref_models", "/root/reference/tools/models.py")
ref_models = importlib.util.module_from_spec(spec)
spec.loader.exec_module(ref_models)

torch.set_num_threads(1)
torch.Tensor.cuda = lambda self, *a, **k: self.clone()

out = {}
for name in DC.GOLDEN:
    case = DC.CASE[name]
    lists = [[torch.from_numpy(p[k]).requires_grad_(True) for p in case["preds"]] for k in range(3)]
    if not case["multi"]:                    # the function reads segm_preds[1] before it looks at multi_scale
        for k, ch in enumerate((1, 2, 4)):
            lists[k].append(torch.zeros(case["N"], ch, 1, 1))
    gt = [torch.from_numpy(v) for v in case["gt"]]
    stub = types.SimpleNamespace(angle_loss=torch.nn.MSELoss(), multi_scale=case["multi"])
    total = ref_models.ModelResNetSep2.loss(stub, lists[0], gt[0], gt[1], lists[1], gt[2], lists[2], gt[3])
    total.backward()
    terms = [stub.segm_loss_value, stub.angle_loss_value, stub.box_loss_value, total]
    out[name + ".terms"] = np.array([float(t.detach()) for t in terms], dtype=np.float32)
    for k, tag in enumerate(("segm", "angle", "roi")):
        for s, p in enumerate(case["preds"]):
            out["%s.%s%d" % (name, tag, 4 << s)] = p[k]
            out["%s.grad_%s%d" % (name, tag, 4 << s)] = lists[k][s].grad.numpy()
    for tag, v in zip(("segm_gt", "iou_mask", "angle_gt", "roi_gt"), case["gt"]):
        out["%s.%s" % (name, tag)] = v
    print(name, out[name + ".terms"])
np.savez_compressed(os.path.join(HERE, "detection_loss.npz"), **out)
print("wrote detection_loss.npz:", os.path.getsize(os.path.join(HERE, "detection_loss.npz")), "bytes")
