"""`tbn_clip_summary` / `ops.clip_summary` at operator level against the fp64 restatement of tests/vis_summary_ref.py:
indices exact, probabilities and entropies within bounds derived from fp32 rounding (stated there).

Observed on an MI355X (scripts/vis_info_profile.py -> profiles/vis_summary.md): largest error / bound 0.231 for the
probabilities and 0.199 for the entropies over the cases of `R.cases()`."""
import ctypes

import numpy as np
import pytest
import torch

from tests import vis_summary_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"


def test_every_case_against_the_fp64_restatement():
    worst_p, worst_e = 0.0, 0.0
    for n, case in enumerate(R.cases()):
        p, e = R.check_case(case, R.run_case(case, 100 + n, DEV))
        print("case", n, case, "prob error/bound %.3f entropy error/bound %.3f" % (p, e))
        worst_p, worst_e = max(worst_p, p), max(worst_e, e)
    print("largest error/bound: probabilities %.3f, entropy %.3f" % (worst_p, worst_e))
    assert worst_p <= 1.0 and worst_e <= 1.0


def test_uniform_rows_have_the_known_entropy():
    from attention_based_tbn_amd import ops
    for T in R.T_SIZES:
        w32 = np.float32(1.0 / T)
        w = torch.full((6, T), float(w32), device=DEV)
        _, _, ent = ops.clip_summary({"a": torch.zeros(2, 3, device=DEV)}, 1, w, 3)
        # -sum_t w log(w + 1e-6) in closed form: log T but for the 1e-6 inside the logarithm, which moves it by <= 1e-6 T
        known = -T * float(w32) * np.log(np.float64(w32) + R.EPS32)
        assert abs(known - np.log(T)) <= 1.001e-6 * T + 1e-6
        bound = 2.0 ** -20 * (1.0 + abs(known))
        got = ent.cpu().numpy().astype(np.float64)
        print("T", T, "entropy", got, "known", known, "log T", np.log(T), "bound", bound)
        assert np.all(np.abs(got - known) <= bound)


def test_top1_is_topk_corrects_prediction():
    from attention_based_tbn_amd import ops
    from attention_based_tbn_amd._lib import call, ptr, stream_ptr
    rng = np.random.RandomState(5)
    for C, extra in ((5, 0), (64, 3), (65, 0), (352, 0), (1000, 8)):
        s = R.score_rows(rng, 8, C)                     # ties, all-equal, NaN entries, -inf entries, +inf: 8 rows, each
        buf = torch.from_numpy(R.pitched(s, extra)).to(DEV)          # with at least one class that ranks
        target = torch.zeros(8, dtype=torch.int64, device=DEV)
        correct = torch.empty((1, 8), dtype=torch.uint8, device=DEV)
        pred = torch.empty((1, 8), dtype=torch.int64, device=DEV)
        call("tbn_topk_correct", ptr(buf), C + extra, ptr(target), 8, C, 1, ptr(correct), ptr(pred), 0, stream_ptr())
        idx, _, _ = ops.clip_summary({"a": buf[:, :C]}, 1)
        assert idx[:, 0, 0].cpu().tolist() == pred[0].cpu().tolist()


def test_two_calls_are_bit_identical():
    for n, case in enumerate(R.cases()[-6:]):
        a, b = R.run_case(case, 7 + n, DEV), R.run_case(case, 7 + n, DEV)
        assert np.array_equal(a[0], b[0])
        assert a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes()
    case = dict(heads=[(125, 0), (1000, 0)], B=9, k=5, weights=(3, 130, 0))
    a, b = R.run_case(case, 3, DEV), R.run_case(case, 3, DEV)
    assert a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes()


def test_ring_offset_leaves_the_other_rows():
    from attention_based_tbn_amd import ops
    rng = np.random.RandomState(9)
    scores = {"verb": torch.from_numpy(R.score_rows(rng, 5, 125, special=False)).to(DEV),
              "noun": torch.from_numpy(R.score_rows(rng, 5, 352, special=False)).to(DEV)}
    w = torch.from_numpy(R.weight_rows(rng, 10, 8)).to(DEV)
    alone = ops.clip_summary(scores, 5, w.unsqueeze(1), 2)               # (R, 1, T) weights
    idx = torch.full((12, 2, 5), -7, dtype=torch.int32, device=DEV)
    prob = torch.full((12, 2, 5), -7.0, device=DEV)
    ent = torch.full((12,), -7.0, device=DEV)
    views = ops.clip_summary(scores, 5, w, 2, out=(idx, prob, ent), row=4)
    for ring, view, ref in zip((idx, prob, ent), views, alone):
        assert view.data_ptr() == ring[4:9].data_ptr() and torch.equal(ring[4:9], ref)
        assert bool((ring[:4] == -7).all()) and bool((ring[9:] == -7).all())
    with pytest.raises(Exception, match="outside rings"):
        ops.clip_summary(scores, 5, w, 2, out=(idx, prob, ent), row=8)


def test_wrapper_refuses_cpu_tensors():
    from attention_based_tbn_amd import ops
    from attention_based_tbn_amd._lib import TbnHipError
    with pytest.raises(TbnHipError, match="no CPU fallback"):
        ops.clip_summary({"a": torch.zeros(2, 3)}, 1)
    with pytest.raises(TbnHipError, match="no CPU fallback"):
        ops.clip_summary({"a": torch.zeros(2, 3, device=DEV)}, 1, torch.zeros(2, 4))


def test_argument_refusals_and_empty_batch():
    from attention_based_tbn_amd._lib import SummaryHead, lib, ptr
    s = torch.zeros((4, 8), device=DEV)
    w = torch.full((8, 8), 0.125, device=DEV)
    idx = torch.full((4, 2, 8), -7, dtype=torch.int32, device=DEV)
    prob = torch.full((4, 2, 8), -7.0, device=DEV)
    ent = torch.full((4,), -7.0, device=DEV)
    fn = lib().tbn_clip_summary

    def heads(*rows):
        arr = (SummaryHead * max(1, len(rows)))()
        for i, (p, ld, C) in enumerate(rows):
            arr[i] = SummaryHead(p, ld, C)
        return arr

    good = heads((ptr(s), 8, 8), (ptr(s), 8, 6))

    def refused(message, *args):
        assert fn(*args, None) != 0
        text = lib().tbn_last_error().decode()
        assert text.startswith("clip_summary: ") and message in text, text

    P = dict(i=ptr(idx), p=ptr(prob), e=ptr(ent), w=ptr(w))
    refused("null argument", None, 2, 4, 1, P["w"], 8, 2, 8, P["i"], P["p"], P["e"])
    refused("null argument", good, 2, 4, 1, P["w"], 8, 2, 8, 0, P["p"], P["e"])
    refused("null argument", good, 2, 4, 1, P["w"], 8, 2, 8, P["i"], 0, P["e"])
    refused("null argument in head 1", heads((ptr(s), 8, 8), (0, 8, 8)), 2, 4, 1, P["w"], 8, 2, 8, P["i"], P["p"], P["e"])
    refused("num_heads 0 outside 1..4", good, 0, 4, 1, P["w"], 8, 2, 8, P["i"], P["p"], P["e"])
    refused("num_heads 5 outside 1..4", good, 5, 4, 1, P["w"], 8, 2, 8, P["i"], P["p"], P["e"])
    refused("k 0 outside 1..8", good, 2, 4, 0, P["w"], 8, 2, 8, P["i"], P["p"], P["e"])
    refused("k 9 outside 1..8", good, 2, 4, 9, P["w"], 8, 2, 8, P["i"], P["p"], P["e"])
    refused("k=7 outside 1..6 of head 1", good, 2, 4, 7, P["w"], 8, 2, 8, P["i"], P["p"], P["e"])
    refused("bad shape of head 0 (C=8, ld=7)", heads((ptr(s), 7, 8)), 1, 4, 1, P["w"], 8, 2, 8, P["i"], P["p"], P["e"])
    refused("bad shape of head 0 (C=0, ld=8)", heads((ptr(s), 8, 0)), 1, 4, 1, P["w"], 8, 2, 8, P["i"], P["p"], P["e"])
    refused("bad shape of the weights (T=8, ld=7)", good, 2, 4, 1, P["w"], 7, 2, 8, P["i"], P["p"], P["e"])
    refused("bad shape of the weights (T=0, ld=8)", good, 2, 4, 1, P["w"], 8, 2, 0, P["i"], P["p"], P["e"])
    refused("segments 0", good, 2, 4, 1, P["w"], 8, 0, 8, P["i"], P["p"], P["e"])
    refused("weights and entropy go together", good, 2, 4, 1, P["w"], 8, 2, 8, P["i"], P["p"], 0)
    refused("weights and entropy go together", good, 2, 4, 1, 0, 0, 1, 0, P["i"], P["p"], P["e"])
    refused("batch -1", good, 2, -1, 1, P["w"], 8, 2, 8, P["i"], P["p"], P["e"])
    # an empty batch succeeds and nothing was written by it or by any refused call
    assert fn(good, 2, 0, 1, P["w"], 8, 2, 8, P["i"], P["p"], P["e"], None) == 0
    torch.cuda.synchronize()
    assert bool((idx == -7).all()) and bool((prob == -7).all()) and bool((ent == -7).all())
    assert ctypes.sizeof(SummaryHead) == 16


def test_fixture_table_through_the_kernel():
    """the committed inputs of the reference's own get_info run (tests/golden/vis_info.*) -> the same table"""
    from attention_based_tbn_amd import ops
    from attention_based_tbn_amd.core.tools.vis import info_table
    from tests.vis_util import Names, check_table, fixture_expectations
    z, (_, _, ent64), meta = fixture_expectations()
    scores = {"verb": torch.from_numpy(z["verb"]).to(DEV), "noun": torch.from_numpy(z["noun"]).to(DEV)}
    weights = torch.from_numpy(z["weights"]).to(DEV).unsqueeze(1)
    idx, _, ent = ops.clip_summary(scores, 1, weights, meta["segments"])
    idx, ent = idx.cpu().numpy(), ent.cpu().numpy()
    _, bound = R.ref_entropy(z["weights"], meta["segments"])
    assert np.all(np.abs(ent.astype(np.float64) - ent64) <= bound)
    df = info_table(meta["table"]["vid_id"], z["gt_verb"], z["gt_noun"], idx[:, 0, 0], idx[:, 1, 0], ent,
                    Names(meta["verbs"], meta["nouns"]))
    check_table(df, meta, atol=bound)       # the reference's fp32 entropies: its own 1e-6 relative, plus the kernel's bound
