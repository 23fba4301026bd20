"""Generator of tests/golden/q_dropout.npz: the Q ensemble's members with first-layer dropout through the reference's OWN code on the
CPU under torch autograd -- one `layers.mlp(K, [hidden, hidden], out, dropout=p)` per member (common/layers.py:94-133), in train mode,
in fp64 and in fp32, with one thread.  `torch.nn.functional.dropout` is patched while a member runs so that it multiplies by the
pinned mask; the patch asserts that it is called exactly once per member, with that p, training=True and the shape of the first
layer's output: what the fixture pins is where the mask sits (between the first Linear and its LayerNorm) and that only layer 0 has
one.  Nothing of the reference is restated here.

The masks are the numpy restatement of the library's kernel (tests/dropout_common.py: mask_model) with two rows overwritten, one all
dropped and one all kept.  Stored: the fp32 inputs ("x", "cot", "mask", the stacked parameters) and, for sum(logits * cot),
"logits.f64" / ".f32", "d_x.*" and "d_<parameter>.*".

    python tools/make_q_dropout_golden.py
"""
import io
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import dropout_common as dc  # noqa: E402


def run(ref, x, masks, dtype):
    f = dc.FIX
    G, T, B, K, M, O, p = f["G"], f["T"], f["B"], f["K"], f["hidden"], f["out"], f["p"]
    t = lambda v: torch.tensor(v, dtype=dtype)  # noqa: E731
    xt = t(x["x"]).requires_grad_(True)
    members, outs = [], []
    for g in range(G):
        seq = ref.layers.mlp(K, [M, M], O, dropout=p).to(dtype).train()
        assert seq[0].dropout is not None and seq[1].dropout is None
        with torch.no_grad():
            for i, (w, b, lw, lb) in enumerate((("w0", "b0", "g0", "be0"), ("w1", "b1", "g1", "be1"))):
                seq[i].weight.copy_(t(x[w][g]))
                seq[i].bias.copy_(t(x[b][g]))
                seq[i].ln.weight.copy_(t(x[lw][g]))
                seq[i].ln.bias.copy_(t(x[lb][g]))
            seq[2].weight.copy_(t(x["w2"][g]))
            seq[2].bias.copy_(t(x["b2"][g]))
        calls, mask = [], t(masks[g])

        def pinned(input, p_=0.5, training=True, inplace=False, _mask=mask, _calls=calls):
            assert p_ == p and training is True and not inplace and tuple(input.shape) == (T, B, M), (p_, training, input.shape)
            _calls.append(1)
            return input * _mask

        saved = torch.nn.functional.dropout
        torch.nn.functional.dropout = pinned
        try:
            outs.append(seq(xt))
        finally:
            torch.nn.functional.dropout = saved
        assert len(calls) == 1, "dropout runs exactly once per member: on the first layer"
        members.append(seq)
    logits = torch.stack(outs)
    (logits * t(x["cot"])).sum().backward()
    n = lambda v: v.detach().numpy().copy()  # noqa: E731
    res = {"logits": n(logits), "d_x": n(xt.grad)}
    for i, (w, b, lw, lb) in enumerate((("w0", "b0", "g0", "be0"), ("w1", "b1", "g1", "be1"))):
        res["d_" + w] = np.stack([n(m[i].weight.grad) for m in members])
        res["d_" + b] = np.stack([n(m[i].bias.grad) for m in members])
        res["d_" + lw] = np.stack([n(m[i].ln.weight.grad) for m in members])
        res["d_" + lb] = np.stack([n(m[i].ln.bias.grad) for m in members])
    res["d_w2"] = np.stack([n(m[2].weight.grad) for m in members])
    res["d_b2"] = np.stack([n(m[2].bias.grad) for m in members])
    return res


def generate():
    from oracle import ref_runner

    ref = ref_runner._import_reference()
    x, masks = dc.fixture_inputs(), dc.fixture_masks()
    res = dict(x)
    res["mask"] = masks
    threads = torch.get_num_threads()
    torch.set_num_threads(1)  # one thread: the same reduction order on every machine
    try:
        for dtype, tag in ((torch.float64, "f64"), (torch.float32, "f32")):
            for k, v in run(ref, x, masks, dtype).items():
                res[f"{k}.{tag}"] = np.ascontiguousarray(v)
    finally:
        torch.set_num_threads(threads)
    return res


def main():
    from oracle import ref_runner

    if not ref_runner.available():
        raise SystemExit("the reference tree is not available: nothing to generate")
    res = generate()
    buf = io.BytesIO()
    np.savez_compressed(buf, **res)
    with open(dc.GOLDEN, "wb") as f:
        f.write(buf.getvalue())
    print(f"wrote {dc.GOLDEN}: {len(buf.getvalue())} bytes, {len(res)} arrays")


if __name__ == "__main__":
    main()
