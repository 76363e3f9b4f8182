"""The eval-mode network of nn.cpp:59-88 restated on PyTorch CPU tensors in float64, a rounding model of the 16-bit
kernels, value heads that are alive, and named alterations of the reference (test infrastructure, CPU only).

Why: W.random_weights draws vbatchnorm's single shift once per net, and for most nets of the suite the whole 8x8 value
plane is then negative on every board: the ReLU outputs zeros and the value row is tanh(valuefc.bias) whatever the
input (DESIGN.md 6.1 has the table).  `live_value_blob` moves the shift to the plane's median and scales valuefc so
that tanh works in its curved range; CASES lists the shapes that reach every forward kernel's value path;
MUTATIONS are the defects a test on these cases must be able to see (tests/test_forward_ref.py proves that it can).

Bounds:  bf16 / f16: 2 x max |forward_rounded - forward64| on the case, per
quantity; f32: max(8 x e32, 1e-6), e32 = max |fp32 C oracle - forward64| on the case."""
import functools

import numpy as np

from kami_amd import _lib as L, weights as W

EPS = 1e-5                 # BatchNorm2d's default (nn.cpp:21)
CHUNK = 128                # boards per convolution call: bounds the im2col buffers of the float64 convolutions
PEAKY = 20.0
ROUND_FACTOR, F32_FACTOR, F32_FLOOR, TEETH = 2.0, 8.0, 1e-6, 3.0


def _torch():
    import torch
    return torch


def _dt(dtype):
    torch = _torch()
    return {None: None, "f32": None, "bf16": torch.bfloat16, "f16": torch.float16}[dtype]


def _rd(t, dt):
    """round to `dt` as the kernels do: an fp32 value (accumulator, folded weight, plane) to nearest-even"""
    torch = _torch()
    return t if dt is None else t.to(torch.float32).to(dt).to(torch.float64)


def _tensors(blob, F, C, R):
    torch = _torch()
    return {k: torch.tensor(v.astype(np.float64)) for k, v in W.split(np.asarray(blob), F, C, R).items()}


def _fold(w, conv, bn):
    """-> (conv weight x gamma / sqrt(var + eps), folded shift): BatchNorm on running statistics"""
    torch = _torch()
    s = w[bn + ".weight"] / torch.sqrt(w[bn + ".running_var"] + EPS)
    return w[conv + ".weight"] * s[:, None, None, None], (w[conv + ".bias"] - w[bn + ".running_mean"]) * s + w[bn + ".bias"]


def _conv(h, wf, sh, pad):
    torch = _torch()
    Fn = torch.nn.functional
    return torch.cat([Fn.conv2d(h[i:i + CHUNK], wf, sh, padding=pad) for i in range(0, h.shape[0], CHUNK)])


def trunk(w, R, x, dt=None):
    """stem + residual tower (nn.cpp:62-70) -> h [B, C, 8, 8]; with `dt` rounded where the kernels store 16 bits"""
    torch = _torch()

    def cbr(h, conv, bn):
        wf, sh = _fold(w, conv, bn)
        return torch.relu(_conv(h, _rd(wf, dt), sh, 1))
    h = _rd(torch.tensor(np.asarray(x, np.float64)).permute(0, 3, 1, 2).contiguous(), dt)
    h = _rd(cbr(h, "conv1", "batchnorm1"), dt)
    for i in range(R):
        r = f"residual{i}"
        t = _rd(cbr(h, r + ".conv1", r + ".batchnorm1"), dt)
        h = _rd(h + cbr(t, r + ".conv2", r + ".batchnorm2"), dt)
    return h


def policy_logits(w, h, dt=None):
    """policyconv + pbatchnorm + ReLU, policyconv2 + bias (nn.cpp:72-77) -> logits [B, 4672] in (y, x, plane) order"""
    torch = _torch()
    wf, sh = _fold(w, "policyconv", "pbatchnorm")
    ph = _rd(torch.relu(_conv(h, _rd(wf, dt), sh, 0)), dt)
    return _conv(ph, _rd(w["policyconv2.weight"], dt), w["policyconv2.bias"], 0).permute(0, 2, 3, 1).flatten(1)


# (a)-(h) of DESIGN.md 6.1: alterations of the float64 reference only.  name -> (kind, argument)
MUTATIONS = {
    "a:fc_col0": ("fc_col", 0), "a:fc_col7": ("fc_col", 7), "a:fc_col56": ("fc_col", 56), "a:fc_col63": ("fc_col", 63),
    "b:transpose": ("transpose", None),
    "c:fc_rows3": ("fc_rows", 3), "c:fc_rows7": ("fc_rows", 7), "c:fc_rows254": ("fc_rows", 254),
    "d:vconv_ch0": ("vconv_ch", 0), "d:vconv_chlast": ("vconv_ch", -1),
    "e:vbn_bias0": ("vbn_bias0", None),
    "f:no_relu": ("no_relu", None),
    "g:fc_bias0": ("fc_bias0", None),
    "h:board_xor1": ("board_xor1", None),
}
SINGLE_ELEMENT = ("a:", "d:")          # one weight element each: below the bf16 bound's reach, carried by f16 and f32


def mutations_for(dtype, B):
    return [m for m in MUTATIONS if not (dtype == "bf16" and m.startswith(SINGLE_ELEMENT)) and not (m == "h:board_xor1" and B < 2)]


def value_head(w, h, mutation=None, taps=None):
    """valueconv + vbatchnorm + ReLU + valuefc + tanh (nn.cpp:83-88) on the trunk's output, all float64 (the kernels keep
    this head in fp32) -> value_full [B, 256].  `mutation`: a key of MUTATIONS."""
    torch = _torch()
    kind, arg = MUTATIONS[mutation] if mutation else (None, None)
    w = dict(w)
    if kind == "fc_col":
        w["valuefc.weight"] = w["valuefc.weight"].clone(); w["valuefc.weight"][:, arg] = 0
    elif kind == "fc_rows":
        w["valuefc.weight"] = w["valuefc.weight"].clone(); w["valuefc.weight"][[arg, arg + 1]] = w["valuefc.weight"][[arg + 1, arg]]
    elif kind == "vconv_ch":
        w["valueconv.weight"] = w["valueconv.weight"].clone(); w["valueconv.weight"][0, arg] = 0
    elif kind == "vbn_bias0":
        w["vbatchnorm.bias"] = torch.zeros_like(w["vbatchnorm.bias"])
    elif kind == "fc_bias0":
        w["valuefc.bias"] = torch.zeros_like(w["valuefc.bias"])
    wf, sh = _fold(w, "valueconv", "vbatchnorm")
    z = _conv(h, wf, sh, 0).flatten(1)                            # [B, 64], square y * 8 + x
    if kind == "transpose":
        z = z.reshape(-1, 8, 8).transpose(1, 2).reshape(-1, 64)
    if taps is not None:
        taps["z"] = z.numpy().copy()
    pre = torch.nn.functional.linear(z if kind == "no_relu" else torch.relu(z), w["valuefc.weight"], w["valuefc.bias"])
    if kind == "board_xor1":
        B = pre.shape[0]
        src = np.arange(B) ^ 1
        src[src >= B] = B - 1
        pre = pre[torch.tensor(src)]
    if taps is not None:
        taps["pre"] = pre.numpy().copy()
    return torch.tanh(pre)


def forward64(blob, F, C, R, x, taps=None, mutation=None):
    """-> (policy, value_full [B, 256], logits), float64 ndarrays; `taps` (a dict) receives z [B, 64], the value plane
    before its ReLU, and pre [B, 256], the row before tanh."""
    torch = _torch()
    w = _tensors(blob, F, C, R)
    h = trunk(w, R, x)
    lg = policy_logits(w, h)
    return torch.softmax(lg, 1).numpy(), value_head(w, h, mutation, taps).numpy(), lg.numpy()


def forward_rounded(blob, F, C, R, x, dtype):
    """The rounding model of the bf16 / f16 kernels: float64 arithmetic on values rounded to `dtype` where the kernels
    store 16 bits (input planes; the BatchNorm-folded weights of the stem, the tower, policyconv and policyconv2; every
    layer's output after its ReLU; the residual sum; policyconv's output).  Unrounded, fp32 in the kernels: the folded
    shifts, policyconv2.bias, the whole value head."""
    torch = _torch()
    w, dt = _tensors(blob, F, C, R), _dt(dtype)
    h = trunk(w, R, x, dt)
    lg = policy_logits(w, h, dt)
    return torch.softmax(lg, 1).numpy(), value_head(w, h).numpy(), lg.numpy()


def _live(blob, F, C, R, w, h):
    """live_value_blob on a trunk output that is already known"""
    taps = {}
    value_head(w, h, taps=taps)
    out = blob.copy()
    d = W.split(out, F, C, R)                                     # views into `out`
    d["vbatchnorm.bias"][...] -= np.float32(np.median(taps["z"]))
    w2 = dict(w, **{"vbatchnorm.bias": _torch().tensor(d["vbatchnorm.bias"].astype(np.float64))})
    value_head(w2, h, taps=taps)
    contrib = taps["pre"] - d["valuefc.bias"][None, :].astype(np.float64)
    d["valuefc.weight"][...] *= np.float32(0.5 / contrib.std())
    return out


def live_value_blob(blob, F, C, R, x):
    """A copy of `blob` with vbatchnorm.bias lowered by the median of the pre-ReLU value plane over the inputs `x`, and
    valuefc.weight scaled so that the pre-tanh contribution (row - bias) has standard deviation 0.5 over boards and
    columns.  Everything else is untouched."""
    w = _tensors(blob, F, C, R)
    return _live(np.asarray(blob, np.float32), F, C, R, w, trunk(w, R, x))


def random_boards(n, seed):
    """Synthetic kh_board records covering every field the encoder reads (tests/test_gpu_parity.py::random_boards)"""
    rng = np.random.default_rng(seed)
    b = np.zeros(n, dtype=L.BOARD_DTYPE)
    code = rng.integers(-12, 12, size=(n, 64))
    for t in range(6):
        for col in range(2):
            m = (code == 2 * t + col)
            bits = (m.astype(np.uint64) << np.arange(64, dtype=np.uint64)).sum(1, dtype=np.uint64)
            b["piece_occ"][:, t] |= bits
            b["color_occ"][:, col] |= bits
    b["ply"] = rng.integers(0, 70000, n)
    b["halfmove_clock"] = rng.integers(0, 200, n)
    b["ctm"] = rng.integers(0, 2, n)
    b["castle_rights"] = rng.integers(0, 16, n)
    return b


# name -> F, C, B, R, blob seed (W.random_weights, peaky 20; F + C + R as elsewhere, or the first of F + C + R + 1000 k
# whose live head meets test_forward_ref.py's liveness and teeth conditions: about one seed in four does), input seed, the dtypes the GPU tests run, and what the shape
# reaches on a 256-CU device (choose_plan / plan_layers / plan_tower; kernel names as traced: DESIGN.md 6.1).
# `records`: inputs are ko.observe(random_boards(B, xseed)) and the GPU side is encode_infer on the records.
# `simple`: KAMI_F32_SIMPLE=1.  `table`: a row of DESIGN.md 6.1's case table (the others serve the copy-out test).
def _c(F, C, B, dtypes=("bf16", "f16"), R=1, seed=None, xseed=None, records=False, simple=False, table=True, reaches=""):
    return dict(F=F, C=C, B=B, R=R, seed=F + C + R if seed is None else seed, xseed=B if xseed is None else xseed, dtypes=tuple(dtypes),
                records=records, simple=simple, table=table, reaches=reaches)


CASES = {
    "t8_f30_b1": _c(30, 64, 1, seed=10095, reaches="tower8_kernel, single-pass stem; one board"),
    "t8_f30_b17": _c(30, 64, 17, ("bf16", "f16", "f32"), seed=2095, reaches="tower8_kernel, odd last group; f32: value_conv_f32_kernel + value_fc_kernel"),
    "t8_c24_b17": _c(30, 24, 17, seed=17055, reaches="tower8_kernel, channels padded to 64"),
    "t8_f33_b17": _c(33, 64, 17, seed=21098, reaches="tower8_kernel, four-pass stem"),
    "t8_f119_b37": _c(119, 64, 37, seed=2184, reaches="tower8_kernel, four-pass stem"),
    "t8_f119_b2049": _c(119, 64, 2049, reaches="tower8_kernel, several board groups per workgroup, dead last board"),
    "t8_records_b17": _c(30, 64, 17, seed=4095, xseed=1017, records=True, reaches="tower8_kernel, fused ingest (encode_infer)"),
    "ly_f200_b17": _c(200, 64, 17, seed=10265, reaches="per-layer plan, value_conv_kernel + value_fc_kernel (CP 64, FP 256)"),
    "ly_c160_b17": _c(30, 160, 17, seed=5191, reaches="per-layer plan, CP 192, value_conv_kernel + value_fc_kernel"),
    "ly_c96_b17": _c(30, 96, 17, seed=31127, reaches="per-layer plan + policy_head4_kernel<T,1> (C padded to 128)"),
    "ly_c256_b17": _c(30, 256, 17, seed=2287, reaches="per-layer plan + policy_head4_kernel<T,2>"),
    "t2b_c128_b257": _c(119, 128, 257, reaches="tower2b_kernel<T,128> + policy_head4_kernel<T,1>, ragged group"),
    "t128_b641": _c(119, 128, 641, reaches="tower128_kernel<T,true>, heads inside the launch"),
    "t2s_c256_b17": _c(119, 256, 17, seed=5376, reaches="tower2s_kernel + policy_head4_kernel<T,2>"),
    "t2b_c256_b257": _c(119, 256, 257, reaches="tower2b_kernel<T,256> + policy_head4_kernel<T,2>"),
    "f32_c128_b17": _c(119, 128, 17, ("f32",), seed=16248, reaches="run_f32: value_conv_f32_kernel + value_fc_kernel"),
    "f32_simple_c24_b17": _c(30, 24, 17, ("f32",), xseed=117, simple=True, reaches="forward_simple: simple_conv_kernel + value_fc_kernel"),
    "copy_b5": _c(30, 64, 5, ("bf16", "f32"), table=False, reaches="copy-out modes, one row"),
    "copy_b300": _c(30, 64, 300, ("bf16", "f32"), seed=1095, table=False, reaches="copy-out modes, entries 256.. from board 1"),
}

# the committed cases whose value head is dead (tests/test_gpu_parity.py: seed F + C + R, peaky 20, inputs seeded with B)
DEAD_CASES = [(30, 24, 1, 7), (33, 64, 1, 5), (200, 64, 1, 3), (30, 256, 2, 5)]


def case_inputs(c):
    if c["records"]:
        from oracle import pyoracle as ko
        boards = random_boards(c["B"], c["xseed"])
        # Pieces and side to move are each record's own draw; ply and half-move clock are the first record's, castling
        # rights are none.  Those three fill 18 of the 30 planes with per-board constants (castling planes hold up to
        # 8) that move a board's whole value plane: with each record's own draw 0 % .. 100 % of a board's squares are
        # positive under ANY single vbatchnorm shift (60 blob seeds x 8 record seeds tried: best 17 % .. 98 %), so rows
        # would again be cut or passed whole.  Every header bit's encoding is pinned bit for bit by
        # test_encode_random_boards_vs_oracle and test_fused_ingest_equals_encode_then_infer.
        boards["ply"], boards["halfmove_clock"], boards["castle_rights"] = boards["ply"][0], boards["halfmove_clock"][0], 0
        return ko.observe(boards).astype(np.float32), boards
    return np.random.default_rng(c["xseed"]).random((c["B"], 8, 8, c["F"]), dtype=np.float32), None


def key(c, dtype):
    """the record_maxima key of a case"""
    tag = "_records" if c["records"] else ("_simple" if c["simple"] else "")
    return f"{dtype}:live/F{c['F']}_{c['R']}x{c['C']}_B{c['B']}{tag}"


@functools.lru_cache(maxsize=None)
def case(name):
    """build_case(CASES[name]), computed once per session, shared by the dtypes and the tests, never modified"""
    return build_case(dict(CASES[name], name=name))


def build_case(c):
    """Blob, inputs, the float64 forward, the bounds of every dtype and the effect of every mutation for one entry of
    CASES.
    -> dict: blob, x, boards, value / logits / logp (float64), z (pre-ReLU plane), bound[dtype][quantity],
    model[dtype][quantity] (the rounding model's own error; f32: e32), effect[mutation] = max |dvalue|."""
    torch = _torch()
    from oracle import pyoracle as ko
    F, C, R, B = c["F"], c["C"], c["R"], c["B"]
    x, boards = case_inputs(c)
    raw = W.random_weights(F, C, R, seed=c["seed"], peaky=PEAKY)
    w = _tensors(raw, F, C, R)
    h = trunk(w, R, x)
    blob = _live(raw, F, C, R, w, h)
    w = _tensors(blob, F, C, R)                                   # the trunk's tensors are unchanged
    taps = {}
    value = value_head(w, h, taps=taps).numpy()
    lg = policy_logits(w, h)
    logp = torch.log_softmax(lg, 1).numpy()
    lg = lg.numpy()
    effect = {m: float(np.abs(value_head(w, h, m).numpy() - value).max()) for m in MUTATIONS if not (m == "h:board_xor1" and B < 2)}

    def errs(v, l):
        l = np.asarray(l, np.float64)
        lp = torch.log_softmax(torch.tensor(l), 1).numpy()
        return dict(value=float(np.abs(v - value).max()), logit=float(np.abs(l - lg).max()), logp=float(np.abs(lp - logp).max()))
    model, bound = {}, {}
    for dtype in ("bf16", "f16"):
        hr = trunk(w, R, x, _dt(dtype))
        model[dtype] = errs(value_head(w, hr).numpy(), policy_logits(w, hr, _dt(dtype)).numpy())
        bound[dtype] = {q: ROUND_FACTOR * e for q, e in model[dtype].items()}
        del hr
    _, ov, ol = ko.forward(blob, F, C, R, x)
    model["f32"] = errs(ov, ol)
    bound["f32"] = {q: max(F32_FACTOR * e, F32_FLOOR) for q, e in model["f32"].items()}
    for a in (blob, x, value, lg, logp):
        a.setflags(write=False)
    return dict(c, blob=blob, x=x, boards=boards, value=value, logits=lg, logp=logp, z=taps["z"], pre=taps["pre"],
                model=model, bound=bound, effect=effect)
