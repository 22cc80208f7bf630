"""ResNet-18 / ResNet-34 (torchvision's basic-block networks): the layer table, the key list, the
synthetic weights and the FLOP count, on the host."""
import numpy as np
import pytest

import resnet_c_amd as R

W = R.weights


def _flops_by_hand(arch):
    """2 x MACs of every convolution plus fc, output sizes tracked block by block."""
    out = lambda n, k, s, p: (n + 2 * p - k) // s + 1
    total, res = 2 * 112 * 112 * 64 * 3 * 49, 56   # stem at 112 x 112, then the max-pool
    for pre, cin, cout, stride, has_ds in W.iter_basic_blocks(arch):
        ho = out(res, 3, stride, 1)
        total += 2 * ho * ho * cout * cin * 9 + 2 * ho * ho * cout * cout * 9
        if has_ds:
            total += 2 * ho * ho * cout * cin
        res = ho
    assert res == 7
    return total + 2 * 512 * 1000


@pytest.mark.parametrize("arch,params,convs,keys,flops", [
    ("resnet18", 11_689_512, 20, 102, 3_628_146_688),
    ("resnet34", 21_797_672, 36, 182, 7_327_522_816),
])
def test_basic_block_layer_table(arch, params, convs, keys, flops):
    assert W.block_kind(arch) == "basic" and W.feature_width(arch) == 512
    assert W.param_count(arch) == params            # torchvision's published counts
    assert len(W.conv_specs(arch)) == convs
    specs = dict(W.tensor_specs(arch))
    assert len(W.tensor_specs(arch)) == keys == len(specs)   # no duplicates
    assert specs["layer1.0.conv2.weight"] == (64, 64, 3, 3)
    assert specs["layer1.0.conv1.weight"] == (64, 64, 3, 3)
    assert specs["layer2.0.conv1.weight"] == (128, 64, 3, 3)
    assert specs["layer2.0.downsample.0.weight"] == (128, 64, 1, 1)
    assert specs["layer2.0.downsample.1.running_var"] == (128,)
    assert specs["layer4.1.bn2.bias"] == (512,)
    assert not any(k.startswith("layer1.0.downsample") for k in specs)
    assert not any(".conv3." in k or ".bn3." in k for k in specs)
    assert specs["fc.weight"] == (1000, 512) and specs["fc.bias"] == (1000,)
    ds = [n for n, *_ in W.conv_specs(arch) if n.endswith("downsample.0")]
    assert ds == ["layer2.0.downsample.0", "layer3.0.downsample.0", "layer4.0.downsample.0"]
    strided = [(n, s) for n, _ci, _co, k, s, _p in W.conv_specs(arch) if s != 1]
    assert strided == [("conv1", 2), ("layer2.0.downsample.0", 2), ("layer2.0.conv1", 2),
                       ("layer3.0.downsample.0", 2), ("layer3.0.conv1", 2),
                       ("layer4.0.downsample.0", 2), ("layer4.0.conv1", 2)]
    assert W.forward_flops(arch) == flops == _flops_by_hand(arch)


def test_bottleneck_tables_unchanged():
    assert W.forward_flops("resnet50") == 8_178_368_512     # bench.py's GFLOP/image
    assert W.param_count("resnet50") == 25_557_032
    assert W.block_kind("resnet152") == "bottleneck" and W.feature_width("resnet101") == 2048
    for arch in ("resnet18", "resnet34", "resnet999"):
        with pytest.raises(ValueError):
            W.depths_of(arch)                              # the bottleneck block counts only
    with pytest.raises(ValueError):
        W.block_kind("resnet999")
    with pytest.raises(ValueError):
        list(W.iter_basic_blocks("resnet50"))


def test_basic_generate_state_and_weights_bin_round_trip(tmp_path):
    a = W.generate_state("resnet18", seed=3)
    b = W.generate_state("resnet18", seed=3)
    assert list(a) == [k for k, _ in W.tensor_specs("resnet18")]
    assert all(np.array_equal(a[k], b[k]) and a[k].dtype == np.float32 for k in a)
    assert not np.array_equal(a["layer1.0.conv1.weight"], W.generate_state("resnet18", seed=4)["layer1.0.conv1.weight"])
    # the block's last batch-norm is damped like a bottleneck's bn3; the others are not
    assert 0.02 <= a["layer3.1.bn2.weight"].min() and a["layer3.1.bn2.weight"].max() < 0.1
    assert a["layer3.1.bn1.weight"].min() >= 0.5
    # keys the bottleneck networks share come out of the unchanged per-key generator
    assert np.array_equal(a["conv1.weight"], W.generate_tensor("conv1.weight", (64, 3, 7, 7), 3))
    W.save_weights_bin(a, str(tmp_path))
    (tmp_path / "layer1.0.bn1.num_batches_tracked").write_bytes(np.zeros(1, np.int64).tobytes())
    back = W.load_weights_bin("resnet18", str(tmp_path))
    assert list(back) == list(a) and all(np.array_equal(back[k], a[k]) for k in a)
    (tmp_path / "fc.weight").write_bytes(np.zeros(2048 * 1000, np.float32).tobytes())  # a ResNet-50 fc
    with pytest.raises(ValueError):
        W.load_weights_bin("resnet18", str(tmp_path))


def test_basic_arch_names_reach_the_native_driver_table():
    assert R.model.ARCH_ID["resnet18"] == 18 and R.model.ARCH_ID["resnet34"] == 34
