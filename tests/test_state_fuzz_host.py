"""The state walk of tests/fuzz/state_fuzz.py discriminates (CPU): its engine over a numpy stand-in for the model, the
heads, the neck and the pooler.  The stand-in implements the Python surface the walk drives and the lifecycle rules
the library documents; its outputs are a deterministic function of (input size, dilation flags, image bytes, output
name) -- a generator seeded from a hash of them -- so a never-reconfigured stand-in gives the same bits, and any
state carried over from another configuration or another call does not.

The unflawed stand-in must pass the committed seeds at the committed step counts with the coverage the tool asserts
(this is where the step counts are validated: coverage is a property of the seed and the step count alone); each of
six seeded flaws, one at a time, must fail the walk within that count."""
import hashlib
import os
import sys

import numpy as np
import pytest

import views as V
from resnet_c_amd import preprocess

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "fuzz"))
import state_fuzz as SF  # noqa: E402

GUARD = V.GUARD


class Refused(RuntimeError):
    """the stand-in's RnError: a documented refusal, nothing changed"""


def conv_out(n, k, s, p):
    return (n + 2 * p - k) // s + 1


def stage_hw(size, flags):
    h, w = (conv_out(conv_out(v, 7, 2, 3), 3, 2, 1) for v in size)
    out = [(h, w)]
    for f in flags:
        s = 1 if f else 2
        h, w = (h - 1) // s + 1, (w - 1) // s + 1
        out.append((h, w))
    return out


class World:
    """what the stand-in objects of one factory share: the flaw and the value cache"""

    def __init__(self, flaw):
        self.flaw, self.cache = flaw, {}

    def rows(self, key, name, digests, shape, dtype=np.float32):
        out = np.empty((len(digests),) + tuple(shape), dtype)
        for i, d in enumerate(digests):
            k = (key, name, d, tuple(shape))
            if k not in self.cache:
                seed = int.from_bytes(hashlib.blake2b(repr((key, name)).encode() + d, digest_size=8).digest(), "little")
                rng = np.random.default_rng(seed)
                self.cache[k] = (rng.standard_normal(shape, dtype=np.float32) if dtype == np.float32 else
                                 rng.integers(0, 3, shape).astype(dtype))
            out[i] = self.cache[k]
        return out


def digest(a):
    return hashlib.blake2b(np.ascontiguousarray(a).tobytes(), digest_size=12).digest()


class Scratch:
    """a head's or a neck's scratch, counted in pixels (images x the pixels of the map it works on, as the library
    sizes it): grows with the batch and the map; a live graph of the model refuses a neck's growth"""

    def __init__(self, world):
        self.world, self.cap, self.last, self.handle = world, 0, {}, True

    def reserve(self, B, pix, model=None):
        self.pix = pix
        if B * pix > self.cap:
            if model is not None and model.graphs:
                raise Refused("scratch growth under a live graph")
            if self.world.flaw == "stale_scratch" and self.cap:
                return                                           # the flaw: sized by the first, smaller call for good
            self.cap = B * pix

    def through(self, name, rows):
        """rows as they come out of the scratch: a flawed one leaves the images beyond its size stale (a larger batch
        runs as sub-batches of 512)"""
        fit = self.cap // self.pix
        if min(len(rows), 512) > fit:
            old = self.last.get(name)
            rows = rows.copy()
            rows[fit:] = old[:1] if old is not None and old.shape[1:] == rows.shape[1:] else 0
        self.last[name] = rows
        return rows

    def close(self):
        self.handle = None


class Head(Scratch):
    def __init__(self, world, kind, cin, classes, dtype):
        super().__init__(world)
        self.kind, self.in_channels, self.classes, self.dtype = kind, cin, classes, dtype


class Neck(Scratch):
    def __init__(self, world, cin, a, dtype):
        super().__init__(world)
        self.in_channels_list, self.out_channels, self.dtype = tuple(cin), a, dtype

    @property
    def names(self):
        return tuple(str(i) for i in range(len(self.in_channels_list))) + ("pool",)

    def level_shape(self, name, h, w):
        return (self.out_channels, (h - 1) // 2 + 1, (w - 1) // 2 + 1) if name == "pool" else (self.out_channels, h, w)


class Pooler:
    output_size, featmap_names = (7, 7), ("0", "1", "2", "3")


class HostView:
    def __init__(self, nbytes):
        self.lo, self.nbytes = GUARD, nbytes
        self.whole = np.full(nbytes + 2 * GUARD, V.OUT_BYTE, np.uint8)
        self.image = self.whole.copy()

    def write(self, rows, arr):
        """rows: a boolean mask over the first axis of arr, the rows this call writes"""
        per = arr[0].nbytes if len(arr) else 0
        raw = self.whole[self.lo:self.lo + self.nbytes].reshape(len(arr), per)
        raw[rows] = np.ascontiguousarray(arr).view(np.uint8).reshape(len(arr), per)[rows]


class Model:
    STAGES = SF.STAGES
    CHANNELS = {"resnet50": (4, 8, 16, 32), "resnet18": (2, 4, 8, 16)}

    def __init__(self, world, arch, dtype, size=(224, 224), flags=(0, 0, 0)):
        self.world, self.arch, self.dtype = world, arch, dtype
        self.size, self.flags = tuple(size), tuple(int(f) for f in flags)
        self.basic = arch == "resnet18"
        self.nstreams, self.streams_set, self.front, self.chain = 2, False, 1, 1
        self.graphs = self.pipelines = 0
        self.cap = 0                                            # images the arenas and the model's own logits hold
        self.tuned, self.poisoned = False, False
        self.stale_key, self.stale_request = None, ()
        self.handle = True

    # ---- properties ---------------------------------------------------------------------------------------------------
    input_size = property(lambda self: self.size)
    dilation = property(lambda self: tuple(bool(f) for f in self.flags))
    classes = 10
    features = property(lambda self: self.CHANNELS[self.arch][3])

    def max_sub_batch(self):
        return 512

    @property
    def stage_shapes(self):
        return self.shapes_at((self.size, self.flags))

    def shapes_at(self, key):
        return {s: (c,) + hw for s, c, hw in zip(self.STAGES, self.CHANNELS[self.arch], stage_hw(*key))}

    def parts(self, B):
        p, least = self.nstreams, 128 if self.dtype == "f32" and not self.streams_set else 64
        while p > 1 and B // p < least:
            p //= 2
        return p

    def _reconfigure(self, size, flags):
        if self.graphs or self.pipelines:
            if self.world.flaw == "refused_dilation_moves_the_key" and flags != self.flags:
                self.flags = flags                               # the flaw: refused, and changed all the same
            raise Refused("a Graph or a Pipeline of this model lives")
        if (size, flags) != (self.size, self.flags):
            if self.world.flaw == "stale_key" and size != self.size:
                self.stale_key = (self.size, self.flags)         # the flaw: the first forward still runs the old one
            self.size, self.flags, self.cap, self.tuned = size, flags, 0, False

    def set_input_size(self, H, W):
        if not (32 <= H <= 2048 and 32 <= W <= 2048):
            raise Refused("sides 32..2048")
        self._reconfigure((int(H), int(W)), self.flags)

    def set_dilation(self, a, b, c):
        if self.basic:
            raise Refused("bottleneck networks only")
        self._reconfigure(self.size, (int(bool(a)), int(bool(b)), int(bool(c))))

    def set_streams(self, n):
        self.nstreams, self.streams_set = (2, False) if n == 0 else (int(n), True)

    def set_front_parts(self, n):
        self.front, self.tuned = int(n), False

    def set_chain(self, on):
        self.chain = int(bool(on))

    def _table(self):
        return np.array([7, self.size[0], self.size[1], *self.flags, self.chain, self.front], np.uint64)

    def export_tuning(self):
        if not self.tuned:
            raise Refused("not tuned")
        return self._table()

    def import_tuning(self, words):
        if not np.array_equal(words, self._table()):
            if self.world.flaw != "import_accepted":
                raise Refused("a table of another model or setting")
            self.poisoned = True                                # the flaw: taken silently, and the tiles change values
        self.tuned = True

    # ---- forwards -----------------------------------------------------------------------------------------------------
    def _enter(self, x):
        x = np.asarray(x)
        if x.dtype == np.uint8:
            assert x.shape[1:] == self.size + (3,), (x.shape, self.size)
            x = preprocess.normalize_u8(x)
        assert x.shape[1:] == (3,) + self.size, (x.shape, self.size)
        need = min(len(x), self.max_sub_batch())
        if need > self.cap:
            if self.graphs:
                raise Refused("arena growth under a live graph")
            self.cap = need
        key, self.stale_key = self.stale_key or (self.size, self.flags), None
        if self.poisoned:
            key = (key, "tiles of another table")
        return key, [digest(img) for img in x]

    def _head(self, key, d, logits=False, features=False, probs=False, topk=0):
        out = {}
        for name, on, shape in (("logits", logits, (self.classes,)), ("features", features, (self.features,)),
                                ("probs", probs, (self.classes,)), ("topk_prob", topk, (topk,)), ("topk_idx", topk, (topk,))):
            if on:
                out[name] = self.world.rows(key, name, d, shape, np.int64 if name == "topk_idx" else np.float32)
        return out

    def _stale(self, key, d):
        """the flaw request_survives: the maps of an earlier forward_maps come back with the next dict"""
        shapes = self.shapes_at(key[0] if self.poisoned else key)
        out = {s: self.world.rows(key, s, d, shapes[s]) for s in self.stale_request}
        self.stale_request = ()
        return out

    def forward(self, x, fused=True):
        key, d = self._enter(x)
        return self.world.rows(key, "logits" if fused else "logits_ops", d, (self.classes,))

    forward_u8 = forward

    def forward_outputs(self, x, **kw):
        kw.pop("fused", None)
        key, d = self._enter(x)
        out = self._stale(key, d)
        out.update(self._head(key, d, **kw))
        return out

    def forward_maps(self, x, stages=SF.STAGES, **kw):
        key, d = self._enter(x)
        shapes = self.shapes_at(key[0] if self.poisoned else key)
        out = {s: self.world.rows(key, s, d, shapes[s]) for s in stages}
        out.update(self._head(key, d, **kw))
        if self.world.flaw == "request_survives":
            self.stale_request = tuple(stages)
        return out

    forward_maps_u8 = forward_maps

    def forward_segment(self, x, head, labels=True, scores=False, **kw):
        if head.in_channels != self.features or head.dtype != self.dtype:
            raise Refused("a head of another width or element type")
        key, d = self._enter(x)
        h, w = self.stage_shapes["layer4"][1:]
        head.reserve(min(len(d), self.max_sub_batch()), h * w)
        size = (key[0] if self.poisoned else key)[0]
        out = self._stale(key, d)
        if labels:
            out["labels"] = head.through("labels", self.world.rows(key, head.kind + ".labels", d, size, np.uint8))
        if scores:
            out["scores"] = head.through("scores", self.world.rows(key, head.kind + ".scores", d, (head.classes,) + size))
        out.update(self._head(key, d, **kw))
        return out

    forward_segment_u8 = forward_segment

    def _pyramid(self, x, neck):
        if neck.in_channels_list != self.CHANNELS[self.arch] or neck.dtype != self.dtype:
            raise Refused("a neck of other channels or another element type")
        need = min(len(x), self.max_sub_batch())
        h, w = self.stage_shapes["layer1"][1:]
        if need * h * w > neck.cap and self.graphs:
            raise Refused("neck scratch growth under a live graph")
        key, d = self._enter(x)
        neck.reserve(need, h * w, self)
        shapes = self.shapes_at(key[0] if self.poisoned else key)
        lv = {}
        for i, name in enumerate(neck.names):
            _, h, w = shapes[self.STAGES[min(i, 3)]]
            lv[name] = neck.through(name, self.world.rows(key, "fpn." + name, d, neck.level_shape(name, h, w)))
        return key, d, lv

    def _pool_rois(self, key, d, rois, neck):
        """(pooled, levels, the rows some part of the call writes): every row by the part that holds its image, the
        rows of an invalid image index by the first part"""
        B, K, a = len(d), len(rois), neck.out_channels
        pooled, levels, written = np.zeros((K, a, 7, 7), np.float32), np.full(K, -1, np.int32), np.ones(K, bool)
        second = np.zeros(B, bool)
        for lo in range(0, B, self.max_sub_batch()):
            nb = min(self.max_sub_batch(), B - lo)
            if self.parts(nb) == 2:
                second[lo + nb // 2:lo + nb] = True
        for r, roi in enumerate(rois):
            b = float(roi[0])
            if not (b == int(b) and 0 <= b < B):
                continue
            box = digest(roi[1:])
            pooled[r] = self.world.rows(key, "pooled", [d[int(b)] + box], (a, 7, 7))[0]
            levels[r] = box[0] % 4
            if self.world.flaw == "second_part_unwritten" and second[int(b)]:
                written[r] = False
        return pooled, levels, written

    def forward_fpn(self, x, neck, stages=SF.STAGES, levels=None, rois=None, pooler=None, roi_levels=False, validate=True, **kw):
        key, d, lv = self._pyramid(x, neck)
        out = self._stale(key, d)
        out.update({n: lv[n] for n in neck.names if levels is None or n in levels})
        out.update(self._head(key, d, **kw))
        if rois is not None:
            pooled, lvl, written = self._pool_rois(key, d, np.asarray(rois, np.float32), neck)
            fill = np.frombuffer(bytes([V.OUT_BYTE]) * 4, np.float32)[0]
            pooled[~written] = fill
            out["pooled"] = pooled
            if roi_levels:
                out["roi_levels"] = lvl
        return out

    forward_fpn_u8 = forward_fpn

    def close(self):
        assert not self.graphs, "graphs captured from the model are still alive"
        self.handle = None


class Graph:
    def __init__(self, m, x):
        m._enter(x)                                              # the capture grows what it needs first
        self.m, self.x = m, x
        m.graphs += 1

    def replay(self):
        return self.m.forward(self.x)

    def close(self):
        if self.m:
            self.m.graphs -= 1
            self.m = None


class Pipeline:
    def __init__(self, m, B, input="f32"):
        if input == "images" and m.size != (224, 224):
            raise Refused("the decoded-image route needs 224 x 224")
        self.m = m
        m.pipelines += 1

    def run(self, batches):
        for x in batches:
            yield self.m.forward(x)

    def close(self):
        if self.m:
            self.m.pipelines -= 1
            self.m = None


class Objects:
    def __init__(self, **kw):
        self.__dict__.update(kw)

    def close(self):
        self.model.close()


class StandIn:
    """the factory of state_fuzz.Walk, in numpy; flaw: one of FLAWS or None"""
    Refused = Refused
    normalize_u8 = staticmethod(preprocess.normalize_u8)

    def __init__(self, arch="resnet50", dtype="f32", flaw=None):
        self.arch, self.dtype, self.dilatable = arch, dtype, arch != "resnet18"
        self.world = World(flaw)

    def inputs(self, n, seed, size):
        return np.random.default_rng(seed).standard_normal((n, 3) + tuple(size), dtype=np.float32)

    def _objects(self, m):
        w, cin, dt = self.world, Model.CHANNELS[self.arch], self.dtype
        odt = "bf16" if dt == "f32" else "f32"
        wrong = {"heads": {"width": Head(w, "fcn", cin[3] * 2, 3, dt), "dtype": Head(w, "fcn", cin[3], 3, odt)},
                 "necks": {"width": Neck(w, [c * 2 for c in cin], 4, dt), "dtype": Neck(w, cin, 4, odt)}}
        return Objects(model=m, fcn=Head(w, "fcn", cin[3], 3, dt), deeplab=Head(w, "deeplab", cin[3], 3, dt),
                       neck=Neck(w, cin, 4, dt), pooler=Pooler(), wrong=wrong)

    def subject(self):
        return self._objects(Model(self.world, self.arch, self.dtype))

    def fresh(self, size, flags):
        """the never-reconfigured stand-in has no flaw; it shares the value cache"""
        clean = World(None)
        clean.cache = self.world.cache
        return StandIn._objects(_Clean(self, clean), Model(clean, self.arch, self.dtype, size, flags))

    graph = staticmethod(Graph)
    pipeline = staticmethod(Pipeline)

    @staticmethod
    def tune(m, x):
        out = m.forward(x)
        m.tuned = True
        return out

    place_out = staticmethod(HostView)

    @staticmethod
    def fetch(view, dtype, what, written):
        lo, hi = view.lo, view.lo + view.nbytes
        assert np.array_equal(view.whole[:lo], view.image[:lo]) and np.array_equal(view.whole[hi:], view.image[hi:]), what
        if written:
            V.check_written(view.whole[lo:hi], np.dtype(dtype).itemsize, what)
        return view.whole[lo:hi].view(dtype).copy()

    @staticmethod
    def forward_rois_raw(m, neck, x, rois, pooler, size, level_views, vp, vl):
        assert tuple(size) == m.size
        key, d, lv = m._pyramid(x, neck)
        pooled, levels, written = m._pool_rois(key, d, rois, neck)
        for name, v in level_views.items():
            v.write(np.ones(len(d), bool), lv[name])
        vp.write(written, pooled)
        vl.write(written, levels)

    @staticmethod
    def anchor(*a):
        pass


class _Clean:
    """a factory's arch and dtype over another world"""

    def __init__(self, factory, world):
        self.arch, self.dtype, self.world = factory.arch, factory.dtype, world


FLAWS = {  # flaw -> the words one of which its failure message must hold
    "stale_key": ("differs from the never-reconfigured model", ": shape ("),     # (a): by the values or by a shape
    "stale_scratch": ("differs from the never-reconfigured model",),             # (b)
    "second_part_unwritten": ("never written",),                                 # (c): the 0xA5 fill, not the values
    "refused_dilation_moves_the_key": ("refused, and yet the model reads",),     # (d)
    "request_survives": (": keys [",),                                           # (e)
    "import_accepted": ("must be refused, and was accepted",),                   # (f)
}


@pytest.mark.parametrize("arch,dtype,seed,steps", SF.COMMITTED, ids=lambda v: str(v))
def test_unflawed_stand_in_passes_with_full_coverage(arch, dtype, seed, steps):
    walk = SF.Walk(StandIn(arch, dtype), seed, invariance=True)
    line = walk.run(steps)                                       # check_coverage runs inside
    assert line.endswith(SF.PHRASE) and f"seed {seed}, {steps} steps" in line
    assert all(len(k) == len(SF.FORWARD_KINDS) for k in walk.key_kinds.values()) and len(walk.key_kinds) >= 4
    assert {("fpn_roi", "parts"), ("fpn_roi", "sub"), ("segment", "parts"), ("segment", "sub")} <= walk.big
    for c in ("hold_graph", "hold_pipeline", "release_graph", "release_pipeline", "input_size_refused", "import_refused",
              "refusal_images_pipeline", "refusal_wrong_head", "refusal_wrong_neck", "forward_refused_under_graph"):
        assert walk.counts.get(c, 0) >= 1, (c, walk.counts)
    assert walk.counts.get("dilation_refused" if arch == "resnet50" else "refusal_dilation_basic", 0) >= 1, walk.counts


def test_the_walk_is_a_function_of_seed_and_steps():
    arch, dtype, seed, steps = SF.COMMITTED[0]
    assert SF.Walk(StandIn(arch, dtype), seed).run(steps) == SF.Walk(StandIn(arch, dtype), seed).run(steps)


@pytest.mark.parametrize("flaw", sorted(FLAWS))
def test_seeded_flaw_fails_the_walk(flaw):
    arch, dtype, seed, steps = SF.COMMITTED[0]
    assert arch == "resnet50"
    with pytest.raises(AssertionError) as e:
        SF.Walk(StandIn(arch, dtype, flaw=flaw), seed).run(steps)
    msg = str(e.value)
    assert any(word in msg for word in FLAWS[flaw]), msg
    # replayable from --seed and --steps: the step index and kind, the key and the history counts
    assert f"state_fuzz seed {seed}: step " in msg and " at key ((" in msg and "after counts {" in msg and "keys {" in msg, msg
    step = int(msg.split(": step ")[1].split(" ")[0])
    assert 0 <= step < steps
