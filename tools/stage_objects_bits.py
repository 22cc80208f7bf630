#!/usr/bin/env python3
"""Every object behind the backbone in two forwards on seeded states, for a comparison of two builds of the library
(RN_HIP_LIB selects the build) bit for bit, and for a kernel trace of each.

    python tools/stage_objects_bits.py OUT_DIR                 (once per library: writes one .npy per output)
    python tools/stage_objects_bits.py --compare PARENT_DIR THIS_DIR

The run, at a 64 x 64 input, 2 images: ResNet-18 with a neck, an RPN, a pooler, a box head, a mask head and a keypoint
head in one forward_fpn(..., masks=("probs", "bits"), keypoints=("keypoints", "heatmaps", "rois", "pooled")), every
level exported; a dilated ResNet-50 with a DeepLab head in one forward_segment(scores and labels).  The comparison:
the same files, the same shapes and types, the same bytes."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SIZE, B = (64, 64), 2


def flat(out, prefix=""):
    got = {}
    for k, v in out.items():
        if isinstance(v, dict):
            got.update(flat(v, f"{prefix}{k}."))
        elif isinstance(v, (list, tuple)):
            got.update({f"{prefix}{k}.{i}": np.asarray(x) for i, x in enumerate(v)})
        else:
            got[prefix + k] = np.asarray(v)
    return got


def run(out_dir):
    import resnet_c_amd as R
    from resnet_c_amd import detection as D
    from resnet_c_amd import fpn as P
    from resnet_c_amd import keypoint as KP
    from resnet_c_amd import mask as MK
    from resnet_c_amd import roi as RO
    from resnet_c_amd import rpn as RP
    from resnet_c_amd import segmentation as S
    from resnet_c_amd import weights as W
    os.makedirs(out_dir, exist_ok=True)
    x = W.generate_input(B, seed=64, hw=SIZE)
    state = W.generate_state("resnet18", seed=2)
    a, res, C, Dn = 64, 2, 5, 10
    m = R.NativeModel("resnet18", state=state, input_size=SIZE)
    neck = P.FeaturePyramidNetwork((64, 128, 256, 512), a, P.generate_fpn_state((64, 128, 256, 512), a, seed=1))
    net = RP.RegionProposalNetwork(a, RP.AnchorGenerator(((16,), (32,), (64,), (128,), (256,)), (0.5, 1.0, 2.0)),
                                   RP.generate_rpn_state(a, 3, seed=3), 100, 60, 0.7)
    bh = D.BoxHead(a, res, 64, C, D.generate_box_head_state(a * res * res, 64, C, seed=6), detections_per_img=Dn)
    mh = MK.MaskHead(a, (64,), 64, C, MK.generate_mask_head_state(a, (64,), 64, C, seed=8), resolution=2)
    kh = KP.KeypointHead(a, (64,), 3, KP.generate_keypoint_head_state(a, (64,), 3, seed=9), resolution=2)
    got = m.forward_fpn(x, neck, rpn=net, pooler=RO.MultiScaleRoIAlign(["0", "1", "2", "3"], res, 2), box_head=bh, mask_head=mh,
                        masks=("probs", "bits"), keypoint_head=kh, keypoints=("keypoints", "heatmaps", "rois", "pooled"))
    outs = flat(got, "fpn.")
    for o in (kh, mh, bh, net, neck, m):
        o.close()
    rates = (2, 12)
    d = R.NativeModel("resnet50", state=W.generate_state("resnet50", seed=2), input_size=SIZE, replace_stride_with_dilation=(0, 1, 1))
    head = S.DeepLabHead(2048, 7, S.generate_deeplab_head_state(2048, 7, 64, rates, seed=4), aspp_channels=64, rates=rates, ctx=d.ctx)
    outs.update(flat(d.forward_segment(x, head, labels=True, scores=True), "segment."))
    head.close()
    d.close()
    for k, v in outs.items():
        np.save(os.path.join(out_dir, k + ".npy"), v)
    print(f"{len(outs)} outputs of {os.environ.get('RN_HIP_LIB') or 'the tree' + chr(39) + 's own library'} in {out_dir}: "
          f"detections {got['detections'].tolist()}, mask bits set {int(np.asarray(got['mask_bits']).sum())}")
    return 0


def compare(a_dir, b_dir):
    a, b = sorted(os.listdir(a_dir)), sorted(os.listdir(b_dir))
    print(f"outputs of the parent's library: {len(a)}; of this one: {len(b)}; the same names: {a == b}")
    wrong = 0 if a == b else 1
    for name in a:
        if name not in b:
            continue
        p, q = np.load(os.path.join(a_dir, name)), np.load(os.path.join(b_dir, name))
        same = p.shape == q.shape and p.dtype == q.dtype and np.array_equal(np.ascontiguousarray(p).view(np.uint8),
                                                                            np.ascontiguousarray(q).view(np.uint8))
        wrong += not same
        print(f"  {name[:-4]:28s} {str(p.dtype):8s} {str(p.shape):20s} {'same bytes' if same else 'DIFFERENT'}")
    print(f"outputs that differ: {wrong}")
    return 1 if wrong else 0


if __name__ == "__main__":
    sys.exit(compare(sys.argv[2], sys.argv[3]) if sys.argv[1] == "--compare" else run(sys.argv[1]))
