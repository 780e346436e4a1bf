"""The host helpers the fleet stages share (mkz_mpc_path_follower_amd/_stage.py): what they return, not what the stages say with them -- the
stages' own texts are tests/test_stage_contracts.py's.  CPU only: the helpers touch no device.
"""
import numpy as np
import pytest
import torch

from mkz_mpc_path_follower_amd import _stage as S

B = 5
CPU = torch.device("cpu")
TEXT = "state: expected [%d,W] with X, Y, psi, v in the first four columns, got %s"


def test_state_view_passes_the_plants_state_without_a_copy():
    """the plant's [B,8] and a column slice of it go to the kernels as they are -- the very object, for every width a stage asks for"""
    state = torch.arange(B * 8, dtype=torch.float64).reshape(B, 8)
    head = state[:, 0:4]
    for c in (2, 3, 4):
        assert S.is_state_view(state, c, CPU) and S.is_state_view(state, c, CPU, rows=B) and not S.is_state_view(state, c, CPU, rows=B + 1)
        assert S.state_view(state, c, CPU, B, TEXT) is state
        assert S.state_view(state, c, CPU, None, "%s") is state
        assert S.is_state_view(head, c, CPU) and S.state_view(head, c, CPU, B, TEXT) is head
    tail = state[:, 4:8]   # a slice that does not start at column 0: rows 8 apart, unit column stride
    assert S.state_view(tail, 4, CPU, B, TEXT) is tail and tail.stride() == (8, 1)
    empty = torch.zeros((0, 8), dtype=torch.float64)
    assert S.state_view(empty, 4, CPU, 0, TEXT) is empty


def test_state_view_copies_what_a_kernel_cannot_read():
    state = torch.arange(B * 8, dtype=torch.float64).reshape(B, 8)
    cases = {
        "column-strided": state[:, ::2],                          # [B,4], columns 2 apart
        "transposed": torch.arange(4 * B, dtype=torch.float64).reshape(4, B).t(),
        "float32": state.float(),
        "rows closer than c": torch.as_strided(torch.arange(B + 3, dtype=torch.float64), (B, 4), (1, 1)),
        "numpy": state.numpy().copy(),
        "lists": state.tolist(),
    }
    for name, x in cases.items():
        if isinstance(x, torch.Tensor):
            assert not S.is_state_view(x, 4, CPU), name
        got = S.state_view(x, 4, CPU, B, TEXT)
        assert got is not x and got.dtype == torch.float64 and got.is_contiguous() and S.is_state_view(got, 4, CPU, rows=B), name
        assert torch.equal(got, torch.as_tensor(x, dtype=torch.float64)), name
    assert S.is_state_view(state[:, ::2], 1, CPU) is False and S.is_state_view(state[:, 0:1], 1, CPU)   # one column of eight: rows 8 apart


def test_state_view_refuses_with_the_sites_text():
    state = torch.zeros((B, 8), dtype=torch.float64)
    for x, shape in ((torch.zeros((B + 1, 8), dtype=torch.float64), "(6, 8)"), (state[:, 0:3], "(5, 3)"), (state.float()[:, 0:3], "(5, 3)"),
                     (np.zeros((2, 8)), "(2, 8)"), (torch.zeros(B, dtype=torch.float64), "(5,)")):
        with pytest.raises(ValueError) as e:
            S.state_view(x, 4, CPU, B, TEXT)
        assert str(e.value) == "state: expected [5,W] with X, Y, psi, v in the first four columns, got " + shape
    with pytest.raises(ValueError) as e:   # no row count asked for: the text takes the shape alone
        S.state_view(state[:, 0:2], 3, CPU, None, "state: expected [B,W] with X, Y, psi in the first three columns, got %s")
    assert str(e.value) == "state: expected [B,W] with X, Y, psi in the first three columns, got (5, 2)"
    assert S.state_view(torch.zeros((B + 1, 8), dtype=torch.float64), 3, CPU, None, "%s").shape == (B + 1, 8)


def test_cap_pair_path_id_and_present():
    v = torch.ones(B, dtype=torch.float64)
    assert S.cap_in(v, B, CPU) is v and S.cap_in([1.0] * B, B, CPU).dtype == torch.float64 and S.cap_in(v.float(), B, CPU).dtype == torch.float64
    assert S.cap_out(v, B, CPU) is v and S.cap_out(None, B, CPU).shape == (B,)
    pid = torch.zeros(B, dtype=torch.int32)
    assert S.own_path_id(pid, B, CPU) is pid
    S.check_present(None, B, CPU), S.check_present(torch.ones(B, dtype=torch.bool), B, CPU), S.check_present(torch.ones(B, dtype=torch.uint8), B, CPU)
    for call, text in ((lambda: S.cap_in(torch.ones(B + 1), B, CPU), "v_cap: expected [5], got (6,)"),
                       (lambda: S.cap_out(v.float(), B, CPU), "out: expected a contiguous float64 tensor [5] on cpu"),
                       (lambda: S.own_path_id(pid.long(), B, CPU), "path_id must stay a contiguous int32 tensor [5] on cpu (write into it in place)"),
                       (lambda: S.check_present(torch.ones(B, dtype=torch.int32), B, CPU), "present: expected a contiguous uint8 or bool tensor [5] on cpu")):
        with pytest.raises(ValueError) as e:
            call()
        assert str(e.value) == text


def test_fresh_record_and_record_fields():
    """one behaviour for the four fresh_* functions: a device index's spelling, a name or a torch.device; the record's words by name"""
    from mkz_mpc_path_follower_amd import ref_traj as RT
    for fresh, words, word, value in ((RT.fresh_score, 16, 15, -1.0), (RT.fresh_follow_stat, 8, 4, float("inf")), (RT.fresh_range_rec, 16, 5, -1.0),
                                      (RT.fresh_lane_rec, 16, 8, float("inf"))):
        for device in ("cpu", CPU):
            rec = fresh(2, device)
            assert rec.shape == (2, words) and rec.dtype == torch.float64 and rec.device == CPU
            assert rec[:, word].tolist() == [value, value] and rec.sum(1).tolist() == [value, value]
    rec = torch.tensor([[1.0, 2.5, 3.0], [4.0, 5.5, 6.0]], dtype=torch.float64)
    out = S.record_fields(rec, ("n", "x", "k"), ("n", "k"))
    assert list(out) == ["n", "x", "k"] and out["n"].dtype == np.int64 and out["k"].tolist() == [3, 6] and out["x"].tolist() == [2.5, 5.5]
    out["x"][0] = 0.0   # copies: the record is not written through them
    assert rec[0, 1].item() == 2.5 and S.record_fields(rec, ("n",))["n"].dtype == np.float64
