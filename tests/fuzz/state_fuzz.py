#!/usr/bin/env python3
"""Randomised walk over the model driver's whole state machine: every property that can change on a live model
(set_input_size, set_dilation, streams, depth-first front, chains, tune, export_tuning / import_tuning), every
forward kind (forward, forward_outputs, forward_maps, forward_segment with an FCN and a DeepLab head, forward_fpn
with and without RoIs, the _u8 twin of each), held Graph / Pipeline objects and the documented refusals, all on ONE
model, ONE head of each kind, ONE neck and ONE pooler.  What is under test is the state they carry from one
configuration and one call into the next: a shape, a capacity, a tuned tile, a request pointer, a scratch slice.

After every forward, bit for bit: every returned array equals what a never-reconfigured model gave for those
images -- a second model with second heads and a second neck from the same states, created at that (input size,
dilation flags), whose only history is one forward per kind over the image pool on one stream; it is closed at
once and its outputs are kept as host arrays.  That model is itself checked once per key against the float64
references, with the helpers and bounds of the feature's own GPU tests (DeviceFactory.anchor).

The walk is an engine (Walk) over a factory of the objects it drives; DeviceFactory makes the device's, and
tests/test_state_fuzz_host.py puts a numpy stand-in with seeded flaws in its place.  It is counted in steps, so a
fixed seed is the same program on every machine; model_fuzz.py covers the full-size configuration by the clock.

    python tests/fuzz/state_fuzz.py [--steps 300] [--seed 0] [--dtype f32|bf16] [--arch resnet50|resnet18]
                                    [--invariance] [--no-anchor]"""
import argparse
import os
import sys

TESTS = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.dirname(TESTS), TESTS):
    if p not in sys.path:
        sys.path.insert(0, p)
import numpy as np

import views as V

PHRASE = "gave the never-reconfigured model's bits"
# the runs of the suite (tests/test_fuzz_gpu.py; tests/test_state_fuzz_host.py validates their coverage on the CPU)
COMMITTED = [("resnet50", "f32", 201, 300), ("resnet50", "bf16", 213, 300), ("resnet18", "f32", 203, 300)]

# (32, 32): final map 1 x 1 (output stride 8: 4 x 4, every ASPP rate centre-only).  (64, 96): fused stem, final map
# 2 x 3.  (44, 64): the fused stem's last partial item.  (104, 72): unfused stem, odd maps (test_input_size_gpu.py)
SIZES = ((32, 32), (64, 96), (44, 64), (104, 72))
FLAGS = ((0, 0, 0), (0, 0, 1), (0, 1, 1), (1, 1, 1))
SMALL = (1, 2, 3, 5)
TWO_PARTS = (128, 130)             # at (32, 32) only, once two streams are set
BIG_SIZE = (32, 32)
NF, NU, NBOX = 8, 4, 6             # float images, byte images and boxes per image of a size's pool
TOPK = 5
STAGES = ("layer1", "layer2", "layer3", "layer4")
HEAD_NAMES = ("logits", "features", "probs", "topk_prob", "topk_idx")
BASE_KINDS = ("forward", "outputs", "maps", "segment", "fpn", "fpn_roi")
FORWARD_KINDS = BASE_KINDS + tuple(k + "_u8" for k in BASE_KINDS)
SWITCHES = ("input_size", "dilation", "streams", "front", "chain", "tune", "export", "import")


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


class Pool:
    """The fixed images of one size: NF float images, NU byte images (x holds their normalised form behind the float
    ones, so one reference covers both routes) and NBOX boxes per image."""

    def __init__(self, factory, size):
        H, W = size
        self.size = size
        self.px = np.random.default_rng(2000 + 7 * H + W).integers(0, 256, (NU, H, W, 3), dtype=np.uint8)
        self.x = np.ascontiguousarray(np.concatenate([factory.inputs(NF, 1000 + 7 * H + W, size),
                                                      factory.normalize_u8(self.px)]), dtype=np.float32)
        rng = np.random.default_rng(3000 + 7 * H + W)
        n = (NF + NU) * NBOX
        side = 2.0 ** rng.uniform(1.5, 6, n)                   # boxes on every level of a pooler with a 16-pixel canon
        x1, y1 = rng.uniform(-4, W, n), rng.uniform(-4, H, n)
        self.boxes = np.stack([x1, y1, x1 + side, y1 + side * rng.uniform(0.6, 1.6, n)], axis=1).astype(np.float32)
        self.boxes = self.boxes.reshape(NF + NU, NBOX, 4)
        for a in (self.px, self.x, self.boxes):
            a.setflags(write=False)

    def all_rois(self):
        idx = np.repeat(np.arange(NF + NU, dtype=np.float32), NBOX)[:, None]
        return np.ascontiguousarray(np.concatenate([idx, self.boxes.reshape(-1, 4)], axis=1))


class Walk:
    """The engine.  factory: arch, dtype, dilatable, Refused (the exception a documented refusal raises), inputs,
    normalize_u8, subject() / fresh(size, flags) -> an object with model, fcn, deeplab, neck, pooler, wrong (a dict of
    mismatched heads and necks) and close(); graph / pipeline / tune; place_out / fetch / forward_rois_raw; anchor."""

    def __init__(self, factory, seed, invariance=False, anchor=True, out=None):
        self.f, self.seed = factory, seed
        self.g = np.random.default_rng(seed)
        self.invariance, self.do_anchor = invariance, anchor
        self.say = out or (lambda s: None)
        self.pools, self.refs = {}, {}
        self.counts, self.key_counts, self.pair_counts, self.key_kinds = {}, {}, {}, {}
        self.big = set()                                       # (kind, "parts" | "sub") seen
        self.sub_done = set()
        self.step_no, self.step_kind = -1, "start"
        self.last_switch = "start"
        self.held = None
        self.saved = None                                      # (words, tuning key) of the last export
        self.tuned = False
        self.invariance_log = []

    # ---- the subject and what the walk believes about it ---------------------------------------------------------
    def open(self):
        self.s = self.f.subject()
        self.m = self.s.model
        self.size, self.flags = BIG_SIZE, (0, 0, 0)
        self.m.set_input_size(*self.size)
        self.streams, self.front, self.chain = 1, 1, 1
        self.m.set_streams(1), self.m.set_front_parts(1), self.m.set_chain(1)

    @property
    def key(self):
        return (self.size, self.flags)

    def tuning_key(self):
        return (self.size, self.flags, self.chain, self.front)

    def pool(self, size):
        if size not in self.pools:
            self.pools[size] = Pool(self.f, size)
        return self.pools[size]

    def history(self):
        return f"counts {self.counts}, keys {self.fmt_keys()}"

    def fmt_keys(self):
        return {f"{s[0]}x{s[1]}/{''.join(map(str, d))}": n for (s, d), n in self.key_counts.items()}

    # ---- the never-reconfigured model ---------------------------------------------------------------------------
    def ref(self, key):
        if key in self.refs:
            return self.refs[key]
        size, flags = key
        pool = self.pool(size)
        o = self.f.fresh(size, flags)
        try:
            m, x = o.model, pool.x
            m.set_streams(1)
            r = {"input_size": m.input_size, "dilation": m.dilation, "stage_shapes": m.stage_shapes,
                 "max_sub": m.max_sub_batch(), "classes": m.classes, "features_n": m.features}
            assert r["input_size"] == size and r["dilation"] == tuple(bool(v) for v in flags), (r, key)
            r["levels"] = {}
            for i, name in enumerate(o.neck.names):
                _, h, w = r["stage_shapes"][STAGES[min(i, 3)]]
                r["levels"][name] = o.neck.level_shape(name, h, w)
            r["logits"] = m.forward(x, fused=True)
            if self.f.dtype == "f32":
                r["logits_ops"] = m.forward(x, fused=False)
            outs = m.forward_outputs(x, logits=True, features=True, probs=True, topk=TOPK)
            self.same("fresh forward_outputs logits", outs["logits"], r["logits"])
            r.update({k: outs[k] for k in HEAD_NAMES[1:]})
            r.update(m.forward_maps(x))
            for hk in ("fcn", "deeplab"):
                seg = m.forward_segment(x, getattr(o, hk), labels=True, scores=True)
                r[hk + ".labels"], r[hk + ".scores"] = seg["labels"], seg["scores"]
            rois = pool.all_rois()
            fp = m.forward_fpn(x, o.neck, rois=rois, pooler=o.pooler, roi_levels=True)
            for name in o.neck.names:
                r["fpn." + name] = fp[name]
            r["pooled"] = fp["pooled"].reshape((NF + NU, NBOX) + fp["pooled"].shape[1:])
            r["roi_levels"] = fp["roi_levels"].reshape(NF + NU, NBOX)
            assert not V.unwritten(np.ascontiguousarray(r["pooled"]), 4).size, "the reference holds the fill pattern"
            if self.invariance:
                self.check_invariance(o, pool, r, key)
            if self.do_anchor:
                self.f.anchor(key, o, pool, r, rois, self.say)
        finally:
            o.close()
        for v in r.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        self.refs[key] = r
        return r

    def check_invariance(self, o, pool, r, key):
        """B = 1 against B = pool on the fresh model, per kind: what comparing slices with the pool's rows rests on"""
        m = o.model
        for i in (0, NF + NU - 1):
            x = pool.x[i:i + 1]
            self.same("invariance forward", m.forward(x), r["logits"][i:i + 1])
            got = m.forward_outputs(x, logits=True, features=True, probs=True, topk=TOPK)
            for k in HEAD_NAMES:
                self.same("invariance " + k, got[k], r[k][i:i + 1])
            got = m.forward_maps(x)
            for k in STAGES:
                self.same("invariance " + k, got[k], r[k][i:i + 1])
            for hk in ("fcn", "deeplab"):
                got = m.forward_segment(x, getattr(o, hk), labels=True, scores=True)
                self.same(f"invariance {hk} scores", got["scores"], r[hk + ".scores"][i:i + 1])
                self.same(f"invariance {hk} labels", got["labels"], r[hk + ".labels"][i:i + 1])
            rois = np.concatenate([np.zeros((NBOX, 1), np.float32), pool.boxes[i]], axis=1)
            got = m.forward_fpn(x, o.neck, rois=rois, pooler=o.pooler, roi_levels=True)
            for name in o.neck.names:
                self.same("invariance level " + name, got[name], r["fpn." + name][i:i + 1])
            self.same("invariance pooled", got["pooled"], r["pooled"][i])
            self.same("invariance roi_levels", got["roi_levels"], r["roi_levels"][i])
        self.invariance_log.append(key)
        self.say(f"  invariance {key}: B = 1 equals B = {NF + NU} bit for bit for every kind")

    # ---- comparisons ------------------------------------------------------------------------------------------------
    def same(self, what, got, want):
        got, want = np.asarray(got), np.asarray(want)
        assert got.shape == want.shape, f"{what}: shape {got.shape}, the fresh model's {want.shape}"
        assert got.dtype == want.dtype, f"{what}: dtype {got.dtype}, the fresh model's {want.dtype}"
        if not np.array_equal(bits(got), bits(want)):
            bad = np.flatnonzero((bits(got) != bits(want)).reshape(got.shape[0], -1).any(axis=1)) if got.ndim else [0]
            raise AssertionError(f"{what}: differs from the never-reconfigured model in rows {list(bad[:8])} of {got.shape[0]}")

    def same_dict(self, what, got, want):
        assert list(got) == list(want), f"{what}: keys {list(got)}, expected {list(want)}"
        for k in want:
            self.same(f"{what} [{k}]", got[k], want[k])

    def check_properties(self, what):
        r, m = self.ref(self.key), self.m
        seen = {"input_size": m.input_size, "dilation": m.dilation, "stage_shapes": m.stage_shapes,
                "max_sub": m.max_sub_batch(), "classes": m.classes, "features_n": m.features}
        for k, v in seen.items():
            assert v == r[k], f"{what}: {k} reads {v}, a model created at {self.key} has {r[k]}"
        for i, name in enumerate(self.s.neck.names):
            _, h, w = r["stage_shapes"][STAGES[min(i, 3)]]
            got = self.s.neck.level_shape(name, h, w)
            assert got == r["levels"][name], f"{what}: level {name} {got}, a fresh neck's {r['levels'][name]}"

    # ---- forwards -----------------------------------------------------------------------------------------------------
    def head_wants(self, some=0.25):
        """the head outputs a maps / segment / fpn forward also asks for, now and then"""
        if self.g.random() >= some:
            return {}
        pick = {"logits": True} if self.g.random() < 0.5 else {"features": True, "topk": TOPK}
        return pick

    def head_rows(self, r, idx, kw):
        out = {}
        for k in HEAD_NAMES:
            asked = kw.get("topk", 0) > 0 if k.startswith("topk") else kw.get(k, False)
            if asked:
                out[k] = r[k][idx]
        return out

    def draw_batch(self, kind, base):
        """(B, what is special about it): the small batches everywhere; at (32, 32) two parts on two streams and, once
        per run for the segment and the FPN-plus-RoI kind, one image more than a launch batch holds"""
        if self.size == BIG_SIZE and not self.held:
            if kind in ("segment", "fpn_roi") and kind not in self.sub_done:
                self.sub_done.add(kind)
                return self.ref(self.key)["max_sub"] + 1, "sub"
            want = base in ("segment", "fpn_roi") and (base, "parts") not in self.big
            if self.streams in (2, 4) and self.g.random() < (0.8 if want else 0.2):
                return int(self.g.choice(TWO_PARTS)), "parts"
        return int(self.g.choice(SMALL)), ""

    def forward_step(self, kind):
        base, u8 = (kind[:-3], True) if kind.endswith("_u8") else (kind, False)
        B, special = self.draw_batch(kind, base)
        n, first = (NU, NF) if u8 else (NF, 0)
        idx = first + (int(self.g.integers(n)) + np.arange(B)) % n
        pool, r, m = self.pool(self.size), self.ref(self.key), self.m
        x = pool.px[idx - NF] if u8 else pool.x[idx]
        what = f"{kind} B={B}"
        if special == "parts":
            assert m.parts(B) == 2, f"{what}: parts({B}) = {m.parts(B)} with {self.streams} streams set"
        if special == "sub":
            assert m.max_sub_batch() + 1 == B, (m.max_sub_batch(), B)
        try:
            getattr(self, "fw_" + base)(what, m, r, pool, x, idx, u8, special)
        except self.f.Refused:
            if not (self.held and self.held["kind"] == "graph"):
                raise
            self.count("forward_refused_under_graph")           # growth under a live graph: refused, nothing changed
            self.check_properties(what + " after a refused growth")
            return
        self.check_properties(what)
        self.counts[kind] = self.counts.get(kind, 0) + 1
        self.key_counts[self.key] = self.key_counts.get(self.key, 0) + 1
        self.key_kinds.setdefault(self.key, set()).add(kind)
        self.pair_counts[(self.last_switch, kind)] = self.pair_counts.get((self.last_switch, kind), 0) + 1
        if special:
            self.big.add((base, special))

    def fw_forward(self, what, m, r, pool, x, idx, u8, special):
        self.same(what, m.forward_u8(x) if u8 else m.forward(x, fused=True), r["logits"][idx])
        if self.f.dtype == "f32" and self.g.random() < 0.3:
            got = m.forward_u8(x, fused=False) if u8 else m.forward(x, fused=False)
            self.same(what + " op by op", got, r["logits_ops"][idx])

    def fw_outputs(self, what, m, r, pool, x, idx, u8, special):
        kw = {"logits": bool(self.g.random() < 0.5), "features": bool(self.g.random() < 0.5),
              "probs": bool(self.g.random() < 0.5), "topk": TOPK if self.g.random() < 0.5 else 0}
        if not (kw["logits"] or kw["features"] or kw["probs"] or kw["topk"]):
            kw["features"] = True
        self.same_dict(what, m.forward_outputs(x, **kw), self.head_rows(r, idx, kw))

    def fw_maps(self, what, m, r, pool, x, idx, u8, special):
        stages = [s for s in STAGES if self.g.random() < 0.5] or [STAGES[int(self.g.integers(4))]]
        self.g.shuffle(stages)
        kw = self.head_wants()
        want = {s: r[s][idx] for s in stages}
        want.update(self.head_rows(r, idx, kw))
        got = m.forward_maps_u8(x, stages, **kw) if u8 else m.forward_maps(x, stages, **kw)
        self.same_dict(f"{what} {stages}", got, want)

    def fw_segment(self, what, m, r, pool, x, idx, u8, special):
        hk = "fcn" if self.g.random() < 0.5 else "deeplab"
        labels, scores = ((True, False), (False, True), (True, True))[int(self.g.integers(3))]
        if special == "sub":
            labels, scores = True, bool(self.g.random() < 0.5)
        kw = self.head_wants()
        want = {}
        if labels:
            want["labels"] = r[hk + ".labels"][idx]
        if scores:
            want["scores"] = r[hk + ".scores"][idx]
        want.update(self.head_rows(r, idx, kw))
        fn = m.forward_segment_u8 if u8 else m.forward_segment
        self.same_dict(f"{what} {hk}", fn(x, getattr(self.s, hk), labels=labels, scores=scores, **kw), want)

    def fw_fpn(self, what, m, r, pool, x, idx, u8, special):
        names = self.s.neck.names
        levels = None if self.g.random() < 0.3 else ([n for n in names if self.g.random() < 0.5] or [names[-1]])
        kw = self.head_wants()
        want = {n: r["fpn." + n][idx] for n in names if levels is None or n in levels}
        want.update(self.head_rows(r, idx, kw))
        fn = m.forward_fpn_u8 if u8 else m.forward_fpn
        self.same_dict(f"{what} levels={levels}", fn(x, self.s.neck, STAGES, levels, **kw), want)

    def draw_rois(self, pool, r, idx, invalid):
        """RoIs of images all over the batch (the first, the last and both halves), a few rows that name no image"""
        B = len(idx)
        K = 24 if B <= 5 else 96
        b = self.g.integers(0, B, K)
        b[:4] = (0, B - 1, B // 2, max(B // 2 - 1, 0))
        box = self.g.integers(0, NBOX, K)
        rois = np.concatenate([b[:, None].astype(np.float32), pool.boxes[idx[b], box]], axis=1)
        pooled, lv = r["pooled"][idx[b], box].copy(), r["roi_levels"][idx[b], box].copy()
        if invalid:
            rows = [5, 11, 17]
            rois[rows, 0] = [B, -1, 0.5]
            pooled[rows], lv[rows] = 0, -1
        return np.ascontiguousarray(rois), pooled, lv

    def fw_fpn_roi(self, what, m, r, pool, x, idx, u8, special):
        names = self.s.neck.names
        raw = bool(special) or self.g.random() < 0.6
        rois, pooled, lv = self.draw_rois(pool, r, idx, invalid=raw or self.g.random() < 0.5)
        if raw:      # the caller's own buffers: 0xA5-filled between guard bands, every element written by this call
            name = names[int(self.g.integers(len(names)))]
            shape = (len(idx),) + r["levels"][name]
            vlev = self.f.place_out(int(np.prod(shape)) * 4)
            vp, vl = self.f.place_out(pooled.size * 4), self.f.place_out(lv.size * 4)
            self.f.forward_rois_raw(m, self.s.neck, x, rois, self.s.pooler, self.size, {name: vlev}, vp, vl)
            got = {name: self.f.fetch(vlev, np.float32, f"{what} level {name}", True).reshape(shape),
                   "pooled": self.f.fetch(vp, np.float32, what + " pooled", True).reshape(pooled.shape),
                   "roi_levels": self.f.fetch(vl, np.int32, what + " roi_levels", True)}
            self.same_dict(what + " raw", got, {name: r["fpn." + name][idx], "pooled": pooled, "roi_levels": lv})
            return
        levels = () if self.g.random() < 0.3 else ([n for n in names if self.g.random() < 0.4] or None)
        with_lv = bool(self.g.random() < 0.5)
        kw = self.head_wants()
        want = {n: r["fpn." + n][idx] for n in names if levels is None or n in levels}
        want.update(self.head_rows(r, idx, kw))
        want["pooled"] = pooled
        if with_lv:
            want["roi_levels"] = lv
        fn = m.forward_fpn_u8 if u8 else m.forward_fpn
        got = fn(x, self.s.neck, STAGES, levels, rois=rois, pooler=self.s.pooler, roi_levels=with_lv, validate=False, **kw)
        self.same_dict(f"{what} levels={levels}", got, want)

    def plain_check(self, what):
        """one image through the plain forward: what a refusal or a closed object must have left alone"""
        i = int(self.g.integers(NF))
        self.same(what, self.m.forward(self.pool(self.size).x[i:i + 1], fused=True), self.ref(self.key)["logits"][i:i + 1])
        self.check_properties(what)

    # ---- property switches ------------------------------------------------------------------------------------------
    def must_refuse(self, what, fn):
        before = (self.m.input_size, self.m.dilation, self.m.stage_shapes)
        try:
            fn()
        except self.f.Refused:
            pass
        else:
            raise AssertionError(f"{what}: must be refused, and was accepted")
        after = (self.m.input_size, self.m.dilation, self.m.stage_shapes)
        assert after == before, f"{what}: refused, and yet the model reads {after}, before {before}"
        self.check_properties(what)

    def may_leave(self):
        """a key is left once every kind has run under it, and not in the run's last steps"""
        if self.size == BIG_SIZE and not all((k, b) in self.big for k in ("segment", "fpn_roi") for b in ("parts", "sub")):
            return False                                        # nor (32, 32) before its large batches have run
        return len(self.key_kinds.get(self.key, ())) == len(FORWARD_KINDS) and self.steps - self.step_no > 50

    def sw_input_size(self):
        size = SIZES[int(self.g.integers(len(SIZES)))]
        if not self.held and not self.may_leave():
            size = self.size                                    # the same value: the setter's early way out
        elif not self.held and size == self.size and self.g.random() < 0.8:
            size = SIZES[(SIZES.index(size) + 1 + int(self.g.integers(len(SIZES) - 1))) % len(SIZES)]
        if self.held and size == self.size:                     # (the library refuses that too, and need not)
            size = SIZES[(SIZES.index(size) + 1) % len(SIZES)]
        if self.held:
            self.count("input_size_refused")
            return self.must_refuse(f"set_input_size{size} under a live {self.held['kind']}", lambda: self.m.set_input_size(*size))
        self.m.set_input_size(*size)
        if size != self.size:
            self.tuned = False
        self.size = size
        self.switched("input_size")

    def sw_dilation(self):
        flags = FLAGS[int(self.g.integers(len(FLAGS)))]
        if not self.held and not self.may_leave():
            flags = self.flags
        elif not self.held and flags == self.flags and self.g.random() < 0.8:
            flags = FLAGS[(FLAGS.index(flags) + 1 + int(self.g.integers(len(FLAGS) - 1))) % len(FLAGS)]
        if self.held and flags == self.flags:
            flags = FLAGS[(FLAGS.index(flags) + 1) % len(FLAGS)]
        if self.held:
            self.count("dilation_refused")
            return self.must_refuse(f"set_dilation{flags} under a live {self.held['kind']}", lambda: self.m.set_dilation(*flags))
        self.m.set_dilation(*flags)
        if flags != self.flags:
            self.tuned = False
        self.flags = flags
        self.switched("dilation")

    def wants_two_parts(self):
        return self.size == BIG_SIZE and not all((k, "parts") in self.big for k in ("segment", "fpn_roi"))

    def sw_streams(self):
        self.streams = int(self.g.choice([2, 4] if self.wants_two_parts() and self.streams not in (2, 4) else [1, 2, 4, 0]))
        self.m.set_streams(self.streams)
        self.switched("streams")

    def sw_front(self):
        self.front = int(self.g.choice([1, 2, 4]))
        self.m.set_front_parts(self.front)
        self.tuned = False                                      # the library drops the table with the setting
        self.switched("front")

    def sw_chain(self):
        self.chain = int(self.g.integers(2))
        self.m.set_chain(self.chain)
        self.switched("chain")

    def sw_tune(self):
        B = int(self.g.choice(SMALL))
        idx = (int(self.g.integers(NF)) + np.arange(B)) % NF
        self.same(f"tune B={B}", self.f.tune(self.m, self.pool(self.size).x[idx]), self.ref(self.key)["logits"][idx])
        self.tuned = True
        self.switched("tune")

    def sw_export(self):
        if not self.tuned:      # no table: the export is refused, then a tune makes one
            self.must_refuse("export_tuning of a model that holds no tuned table", self.m.export_tuning)
            return self.sw_tune_then("export")
        self.saved = (self.m.export_tuning(), self.tuning_key())
        self.switched("export")

    def sw_tune_then(self, then):
        self.sw_tune()
        self.saved = (self.m.export_tuning(), self.tuning_key())
        self.switched(then)

    def sw_import(self):
        if self.saved is None:
            return self.sw_tune_then("export")
        words, tkey = self.saved
        if tkey != self.tuning_key():      # a table of another size, dilation, chain or front setting: refused
            self.count("import_refused")
            self.must_refuse(f"import_tuning of a table of {tkey} at {self.tuning_key()}", lambda: self.m.import_tuning(words))
            self.plain_check("after a refused import_tuning")
            self.sw_tune_then("export")
            words, tkey = self.saved
            self.m.set_front_parts(self.front)                  # drops the table the model holds; the words stay good
            self.must_refuse("export_tuning behind set_front_parts", self.m.export_tuning)
        self.m.import_tuning(words)
        self.tuned = True
        assert np.array_equal(self.m.export_tuning(), words), "export_tuning after import_tuning: not the words imported"
        self.switched("import")

    def switched(self, kind):
        self.last_switch = kind
        self.check_properties(kind)

    # ---- held objects -------------------------------------------------------------------------------------------------
    def hold(self):
        kind = "graph" if self.g.random() < 0.6 else "pipeline"
        B = int(self.g.choice(SMALL + ((130,) if self.size == BIG_SIZE and self.streams in (2, 4) else ())))
        x = self.pool(self.size).x
        if kind == "graph" and self.g.random() < 0.5:
            B = 1                                               # the forwards under it then have something to grow
        if kind == "graph":
            idx = (int(self.g.integers(NF)) + np.arange(B)) % NF
            obj = self.f.graph(self.m, x[idx])
        else:
            idx = [(int(self.g.integers(NF)) + np.arange(n)) % NF for n in (B, B, max(B - 1, 1))]   # a ragged last batch
            obj = self.f.pipeline(self.m, B)
        self.held = {"kind": kind, "obj": obj, "idx": idx, "ttl": int(self.g.integers(2, 7)), "key": self.key}
        self.count("hold_" + kind)

    def release(self):
        h, self.held = self.held, None
        assert h["key"] == self.key, f"the key moved from {h['key']} to {self.key} under a live {h['kind']}"
        r, x = self.ref(self.key), self.pool(self.size).x
        try:
            if h["kind"] == "graph":
                for _ in range(2):
                    self.same("graph replay", h["obj"].replay(), r["logits"][h["idx"]])
            else:
                outs = list(h["obj"].run([x[i] for i in h["idx"]]))
                assert len(outs) == len(h["idx"])
                for got, i in zip(outs, h["idx"]):
                    self.same("pipelined batch", got, r["logits"][i])
        finally:
            h["obj"].close()
        self.count("release_" + h["kind"])
        self.plain_check(f"the forward behind a closed {h['kind']}")

    # ---- refusals that must leave no trace --------------------------------------------------------------------------
    def refusal(self):
        x = self.pool(self.size).x[:2]
        kinds = ["images_pipeline", "wrong_head", "wrong_neck"] + ([] if self.f.dilatable else ["dilation_basic"] * 2)
        kind = kinds[int(self.g.integers(len(kinds)))]
        if kind == "dilation_basic":
            self.must_refuse("set_dilation on a basic-block network", lambda: self.m.set_dilation(0, 1, 1))
        elif kind == "images_pipeline":
            self.must_refuse(f'Pipeline(input="images") at {self.size}', lambda: self.f.pipeline(self.m, 2, input="images"))
        elif kind == "wrong_head":
            for name, head in self.s.wrong["heads"].items():
                self.must_refuse(f"forward_segment with a head of another {name}",
                                 lambda: self.m.forward_segment(x, head, labels=True, scores=True))
        else:
            for name, neck in self.s.wrong["necks"].items():
                self.must_refuse(f"forward_fpn with a neck of another {name}", lambda: self.m.forward_fpn(x, neck))
        self.count("refusal_" + kind)
        self.plain_check(f"the forward behind the refusal {kind}")

    # ---- the walk -----------------------------------------------------------------------------------------------------
    def count(self, kind):
        self.counts[kind] = self.counts.get(kind, 0) + 1

    def switches(self):
        return [s for s in SWITCHES if s != "dilation" or self.f.dilatable]

    def draw_forward(self):
        """uncovered kinds under this key and uncovered (switch, kind) pairs weigh more: the same program per seed"""
        seen = self.key_kinds.get(self.key, ())
        w = np.array([1.0 + 8.0 * (k not in seen) + 4.0 * ((self.last_switch, k) not in self.pair_counts and
                                                              self.last_switch != "start") for k in FORWARD_KINDS])
        return FORWARD_KINDS[int(self.g.choice(len(FORWARD_KINDS), p=w / w.sum()))]

    def draw_switch(self):
        sw = self.switches()
        if self.held:
            sw = [s for s in sw if s not in ("tune", "export", "import")]
        need = {s: sum((s, k) not in self.pair_counts for k in FORWARD_KINDS) for s in sw}
        w = np.array([1.0 + need[s] / 3.0 for s in sw])
        if self.wants_two_parts() and self.streams not in (2, 4):
            w[sw.index("streams")] *= 4.0
        if not self.held and self.may_leave():
            for s in ("input_size", "dilation"):
                if s in sw:
                    w[sw.index(s)] *= 3.0
        return sw[int(self.g.choice(len(sw), p=w / w.sum()))]

    def step(self):
        if self.held:
            self.held["ttl"] -= 1
            if self.held["ttl"] <= 0:
                self.step_kind = "release"
                return self.release()
        u = self.g.random()
        open_pairs = self.last_switch != "start" and any((self.last_switch, k) not in self.pair_counts for k in FORWARD_KINDS)
        if u < (0.75 if open_pairs else 0.5):
            self.step_kind = self.draw_forward()
            return self.forward_step(self.step_kind)
        if u < 0.86:
            self.step_kind = self.draw_switch()
            self.count("set_" + self.step_kind)
            return getattr(self, "sw_" + self.step_kind)()
        if u < 0.93 and not self.held:
            self.step_kind = "hold"
            return self.hold()
        self.step_kind = "refusal"
        return self.refusal()

    def run(self, steps):
        self.steps = steps
        self.open()
        try:
            for self.step_no in range(steps):
                try:
                    self.step()
                except Exception as e:
                    raise AssertionError(f"state_fuzz seed {self.seed}: step {self.step_no} ({self.step_kind}) at key {self.key}, "
                                         f"streams {self.streams}, front {self.front}, chain {self.chain}, held "
                                         f"{self.held and self.held['kind']}: {type(e).__name__}: {e}\n  after {self.history()}") from e
            if self.held:
                self.step_no, self.step_kind = steps, "release"
                try:
                    self.release()
                except Exception as e:
                    raise AssertionError(f"state_fuzz seed {self.seed}: the last release at key {self.key}: {e}\n  after "
                                         f"{self.history()}") from e
        finally:
            if self.held:
                self.held["obj"].close()
                self.held = None
            self.s.close()
        self.check_coverage(steps)
        return self.summary(steps)

    def check_coverage(self, steps):
        where = f"state_fuzz seed {self.seed}, {steps} steps"
        for key, kinds in self.key_kinds.items():
            missing = [k for k in FORWARD_KINDS if k not in kinds]
            assert not missing, f"{where}: at key {key} no forward of kind {missing}"
        missing = [(s, k) for s in self.switches() for k in FORWARD_KINDS if (s, k) not in self.pair_counts]
        assert not missing, f"{where}: {len(missing)} (switch, forward) pairs never ran, the first {missing[:6]}"
        missing = [p for p in (("fpn_roi", "parts"), ("fpn_roi", "sub"), ("segment", "parts"), ("segment", "sub")) if p not in self.big]
        assert not missing, f"{where}: no two-part / two-sub-batch forward of {missing}"

    def summary(self, steps):
        pairs = {f"{s}>{k}": n for (s, k), n in sorted(self.pair_counts.items())}
        return (f"state_fuzz {self.f.arch} {self.f.dtype} seed {self.seed}, {steps} steps: steps {dict(sorted(self.counts.items()))}; "
                f"keys {self.fmt_keys()}; pairs {pairs}: every forward, replay and pipelined batch {PHRASE}")


# =====================================================================================================================
# the device's objects
# =====================================================================================================================
class _Objects:
    def __init__(self, **kw):
        self.__dict__.update(kw)

    def close(self):
        for o in list(self.wrong["heads"].values()) + list(self.wrong["necks"].values()) + [self.fcn, self.deeplab, self.neck]:
            o.close()
        self.model.close()


class _Graph:
    def __init__(self, R, m, x):
        self.R, self.m, self.B = R, m, x.shape[0]
        self.xin = R.FloatTensor.from_numpy(np.ascontiguousarray(x), R.Device.GPU)
        self.out = R.FloatTensor((self.B, m.classes), R.Device.GPU)
        self.g = R.Graph(m, self.xin.data(), self.B, self.out.data(), True)

    def replay(self):
        L = self.R._lib
        L.check(L.lib().rn_memset(self.m.ctx.handle, self.out.data(), 0, self.B * self.m.classes * 4), "memset", self.m.ctx.handle)
        self.g.launch()
        self.m.ctx.sync()
        return self.out.numpy()

    def close(self):
        self.g.close()


class DeviceFactory:
    SEG_CLASSES, ASPP = 21, 64

    def __init__(self, arch, dtype):
        import resnet_c_amd as R
        from resnet_c_amd import fpn, preprocess, roi, segmentation
        from test_fpn_gpu import WIDTH, model_neck_state, stage_channels
        self.R, self.arch, self.dtype = R, arch, dtype
        self.dilatable = arch not in ("resnet18", "resnet34")
        self.Refused = R._lib.RnError
        self.normalize_u8 = preprocess.normalize_u8
        self.state = R.weights.generate_state(arch, seed=0)
        feat = 512 if not self.dilatable else 2048
        self.cin, self.width, self.feat = stage_channels(arch), WIDTH[arch], feat
        self.neck_state = model_neck_state(arch)
        self.fcn_state = segmentation.generate_fcn_head_state(feat, self.SEG_CLASSES, seed=0)
        self.deeplab_state = segmentation.generate_deeplab_head_state(feat, self.SEG_CLASSES, self.ASPP, seed=0)
        other = 2048 if feat == 512 else 512                    # a head and a neck no forward of this model may take
        self.other = other
        self.other_head_state = segmentation.generate_fcn_head_state(other, 3, seed=0, mid_channels=64)
        self.small_head_state = segmentation.generate_fcn_head_state(feat, 3, seed=0, mid_channels=64)
        self.other_cin = tuple(c * 2 for c in self.cin)
        self.other_neck_state = fpn.generate_fpn_state(self.other_cin, 64, seed=2)
        self.small_neck_state = fpn.generate_fpn_state(self.cin, 64, seed=2)
        self.S, self.P, self.RO = segmentation, fpn, roi

    def inputs(self, n, seed, size):
        return self.R.weights.generate_input(n, seed=seed, hw=size)

    def _objects(self, m):
        S, P, dt = self.S, self.P, self.dtype
        odt = "bf16" if dt == "f32" else "f32"
        wrong = {"heads": {"width": S.FCNHead(self.other, 3, self.other_head_state, dtype=dt, mid_channels=64),
                           "dtype": S.FCNHead(self.feat, 3, self.small_head_state, dtype=odt, mid_channels=64)},
                 "necks": {"width": P.FeaturePyramidNetwork(self.other_cin, 64, self.other_neck_state, dtype=dt),
                           "dtype": P.FeaturePyramidNetwork(self.cin, 64, self.small_neck_state, dtype=odt)}}
        return _Objects(model=m, fcn=S.FCNHead(self.feat, self.SEG_CLASSES, self.fcn_state, dtype=dt),
                        deeplab=S.DeepLabHead(self.feat, self.SEG_CLASSES, self.deeplab_state, self.ASPP, dtype=dt),
                        neck=P.FeaturePyramidNetwork(self.cin, self.width, self.neck_state, extra="pool", dtype=dt),
                        pooler=self.RO.MultiScaleRoIAlign(("0", "1", "2", "3"), 7, 2, canonical_scale=16.0, canonical_level=4),
                        wrong=wrong)

    def subject(self):
        return self._objects(self.R.NativeModel(self.arch, state=self.state, dtype=self.dtype))

    def fresh(self, size, flags):
        o = self._objects(self.R.NativeModel(self.arch, state=self.state, dtype=self.dtype, input_size=size,
                                             replace_stride_with_dilation=flags if self.dilatable else None))
        return o

    def graph(self, m, x):
        return _Graph(self.R, m, x)

    def pipeline(self, m, B, input="f32"):
        return self.R.Pipeline(m, B, fused=True, input=input)

    def tune(self, m, x):
        R = self.R
        xin = R.FloatTensor.from_numpy(np.ascontiguousarray(x), R.Device.GPU)
        out = R.FloatTensor((x.shape[0], m.classes), R.Device.GPU)
        m.tune(xin.data(), x.shape[0], out.data(), True)
        m.ctx.sync()
        return out.numpy()

    place_out = staticmethod(V.place_out)

    @staticmethod
    def fetch(view, dtype, what, written):
        return V.fetch(view, dtype, what, written=written)

    def forward_rois_raw(self, m, neck, x, rois, pooler, size, level_views, vp, vl):
        """rn_model_forward_rois(_u8) with the caller's views as pooled, levels_out and the named levels"""
        import ctypes
        L, ops = self.R._lib, self.R.ops
        u8 = x.dtype == np.uint8
        dx = ops._up_raw(np.ascontiguousarray(x, dtype=np.uint8 if u8 else np.float32))
        dr = ops._up_raw(np.ascontiguousarray(rois, dtype=np.float32))
        fo = L.FpnOutputs()
        for name, v in level_views.items():
            fo.level[neck.names.index(name)] = v.ptr
        req = pooler.request(neck.names, dr.ptr, len(rois), size, vp.ptr, vl.ptr)
        fn = L.lib().rn_model_forward_rois_u8 if u8 else L.lib().rn_model_forward_rois
        L.check(fn(m.handle, neck.handle, dx.ptr, x.shape[0], None, (ctypes.c_int * 4)(1, 2, 3, 4), ctypes.byref(fo),
                   ctypes.byref(req), L.RN_FWD_FUSED), "rn_model_forward_rois", m.ctx.handle)
        m.ctx.sync()

    # ---- float64: the fresh model is a kernel result too --------------------------------------------------------------
    def anchor(self, key, o, pool, r, rois, say):
        """The fresh model's outputs of the first two images of the pool against the float64 references, with the
        helpers and bounds of the features' own GPU tests; prints what those print, and error / bound."""
        from oracle import netref as N
        from test_dilation_gpu import tol_bf16, tol_f32
        from test_dilation_host import dilated_features_f64
        from test_fpn_gpu import check_levels
        from test_fpn_host import products
        from test_input_size_gpu import TOL
        from test_roi_gpu import check_pooled_against_f64
        size, flags = key
        n, bf, ops = 2, self.dtype == "bf16", self.R.ops
        x = pool.x[:n]
        tag = f"{self.arch} {self.dtype} {size[0]}x{size[1]}/{''.join(map(str, flags))}"
        rd = ops.bf16_round if bf else None
        if not bf:
            feats = dilated_features_f64(self.arch, self.state, x, flags) if self.dilatable else N.features_f64(self.arch, self.state, x)
            want = N.ref_logits(self.state, feats)
            for name in ("logits", "logits_ops"):
                err = float(np.abs(r[name][:n] - want).max())
                say(f"  anchor {tag}: {name} max|gpu - fp64| = {err:.3e}, error / bound {err / TOL:.3f}")
                assert err <= TOL, (tag, name, err)
        elif self.dilatable:
            self.anchor_bf16_logits(key, tag, say)
        ref = self.P.fpn_ref([r[s][:n].astype(np.float64) for s in STAGES], self.neck_state, "pool", round_fn=rd)
        got = {name: r["fpn." + name][:n] for name in o.neck.names}
        check_levels(got, ref, self.cin, self.width, self.dtype, "state walk " + tag)
        worst = max(float(np.abs(got[str(i)] - ref[str(i)]).max()) /
                    (tol_bf16(ref[str(i)]) if bf else tol_f32(ref[str(i)], products(self.cin, self.width, i)))
                    for i in range(4))
        say(f"  anchor {tag}: pyramid worst error / bound {worst:.3f}")
        sel = np.arange(n * NBOX)
        check_pooled_against_f64(r["pooled"].reshape((-1,) + r["pooled"].shape[2:])[sel], r["roi_levels"].reshape(-1)[sel], ref,
                                 o.pooler.featmap_names, rois[sel], o.pooler, size, self.cin, self.width, self.dtype,
                                 "state walk " + tag)
        l4 = r["layer4"][:n].astype(np.float64)
        for hk, head_ref in (("fcn", lambda: self.S.fcn_head_ref(l4, self.fcn_state, size, round_fn=rd)),
                             ("deeplab", lambda: self.S.deeplab_head_ref(l4, self.deeplab_state, size, round_fn=rd))):
            want = head_ref()
            scores, labels = r[hk + ".scores"][:n], r[hk + ".labels"][:n]
            tol = tol_bf16(want) if bf else tol_f32(want, 9 * self.feat)
            err = float(np.abs(scores - want).max())
            say(f"  anchor {tag}: {hk} scores max|gpu - fp64 head on the gpu's map| = {err:.3e}, error / bound {err / tol:.3f}")
            assert scores.shape == want.shape and err <= tol, (tag, hk, err, tol)
            assert np.array_equal(r[hk + ".labels"], r[hk + ".scores"].argmax(axis=1)), (tag, hk, "labels are not the argmax")
            assert labels.dtype == np.uint8

    def anchor_bf16_logits(self, key, tag, say):
        """bf16 logits as test_input_size_gpu.py / test_dilation_gpu.py check them: a model with the fc re-centred to a
        logit spread of 1 on structured images, within 2.3 times the CPU emulation's own distance from float64"""
        from oracle import netref as N
        from test_dilation_gpu import features_bf16_emulated, structured
        from test_dilation_host import dilated_features_f64
        size, flags = key
        finch = np.fromfile(os.path.join(TESTS, "golden", "finch_224.bin"), dtype=np.float32).reshape(1, 3, 224, 224)
        x = structured(finch, size)
        st, want = N.recentre_fc(self.state, dilated_features_f64(self.arch, self.state, x, flags), spread=1.0)
        emu = N.logits_bf16_emulated(st, features_bf16_emulated(self.arch, st, x, flags))
        dist, spread = float(np.abs(emu - want).max()), N.logit_spread(want)
        bound = 2.3 * dist
        m = self.R.NativeModel(self.arch, state=st, dtype="bf16", input_size=size, replace_stride_with_dilation=flags)
        try:
            got = m.forward(x, fused=True)
        finally:
            m.close()
        err = float(np.abs(got - want).max())
        say(f"  anchor {tag}: bf16 logits: emulation {dist:.4f}, bound {bound:.4f}, spread {spread:.3f}, gpu {err:.4f}, "
            f"error / bound {err / bound:.3f}")
        assert spread > 5 * bound, (tag, bound, spread)
        assert err <= bound, (tag, err, bound)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--dtype", default="f32", choices=["f32", "bf16"])
    ap.add_argument("--arch", default="resnet50", choices=["resnet50", "resnet18"])
    ap.add_argument("--invariance", action="store_true", help="also check B = 1 against B = pool on every fresh model")
    ap.add_argument("--no-anchor", action="store_true", help="skip the float64 anchors of the fresh models")
    a = ap.parse_args()
    walk = Walk(DeviceFactory(a.arch, a.dtype), a.seed, invariance=a.invariance, anchor=not a.no_anchor, out=print)
    print(walk.run(a.steps))


if __name__ == "__main__":
    main()
