"""sixdgs_gaussian_adam and sixdgs_opacity_reset on the GPU: the one-launch Adam kernel against the fp64 restatement
(tests/gaussian_adam_reference.py) under its own fp32 bound over a size matrix, every array between guard bytes; its 16-byte and
4-byte access paths bit for bit against each other; the frozen group, the non-finite entry and the capacity rules; the reset;
determinism.  Everything runs inside this process."""
import importlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gaussian_adam_reference as R  # noqa: E402

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

GUARD = 256


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    importlib.import_module("6dgs_amd")
    return importlib.import_module("6dgs_amd.ops")


def guarded(values, shift=0):
    """(buffer, view): the float32 array `values` on the GPU between two runs of GUARD bytes of 0x5A, its first byte `shift` bytes past
    a 16-byte boundary."""
    values = np.ascontiguousarray(values, np.float32)
    buf = torch.full((values.size * 4 + 2 * GUARD + 16,), 0x5A, dtype=torch.uint8, device="cuda")
    start = GUARD + (shift - (buf.data_ptr() + GUARD)) % 16
    view = buf[start:start + values.size * 4].view(torch.float32)
    assert view.data_ptr() % 16 == shift
    view.copy_(torch.from_numpy(values.reshape(-1)))
    return (buf, start, values.size * 4), view


def guards_intact(handle):
    buf, start, size = handle
    return bool((buf[:start] == 0x5A).all()) and bool((buf[start + size:] == 0x5A).all())


def upload(params, m, v, shift=0):
    """Guarded device copies -> (handles, params dict, state dict)."""
    handles, p = [], {}
    n = params["xyz"].size // 3
    shapes = {"xyz": (n, 3), "f_dc": (n, 1, 3), "f_rest": (n, params["f_rest"].size // (3 * n), 3), "opacity": (n,), "scale": (n, 3), "rot": (n, 4)}
    for k in R.GROUPS:
        h, flat = guarded(params[k], shift)
        p[k] = flat.reshape(shapes[k])
        handles.append(h)
    hm, dm = guarded(m, shift)
    hv, dv = guarded(v, shift)
    state = {"m": dm, "v": dv, "status": torch.zeros(1, dtype=torch.int32, device="cuda")}
    return handles + [hm, hv], p, state


def upload_grads(g, shift=0):
    out = {}
    for k, a in g.items():
        out[k] = None if a is None else guarded(a, shift)[1]
    return out


def within(got, r64, r32, what):
    scale, y, limit = R.bounds({"x": r64}, {"x": r32})["x"]
    a = got.cpu().numpy().astype(np.float64).reshape(-1)
    err = float(np.abs(a - r64).max())
    assert limit <= R.CEILING * scale, f"{what}: the case is unfit"
    assert np.isfinite(a).all() and err <= limit, f"{what}: {err:.3e} > {limit:.3e} (scale {scale:.3e}, y {y:.3e})"
    return err / limit


def bits(t):
    return t.view(torch.int32)


def snapshot(p, state):
    return {**{k: t.reshape(-1).clone() for k, t in p.items()}, "m": state["m"].clone(), "v": state["v"].clone()}


def same_bits(a, b):
    return all(torch.equal(bits(a[k]), bits(b[k])) for k in a)


@pytest.mark.parametrize("n_coef", (1, 4, 16))
@pytest.mark.parametrize("n", (1, 63, 64, 65, 257, 4099))
def test_three_steps_against_fp64(ops, n, n_coef):
    params, m, v, grads = R.random_case(n, n_coef, 0)
    handles, p, state = upload(params, m, v)
    assert p["f_rest"].numel() == 3 * n * (n_coef - 1)                # n_coef = 1: the wrapper passes NULL for the empty group
    for step, g in enumerate(grads):
        ops.gaussian_adam(p, upload_grads(g), state, step, R.LRS, **R.HYPER)
    torch.cuda.synchronize()
    assert all(guards_intact(h) for h in handles), "guard bytes were written"
    assert int(state["status"]) == 0
    p64, m64, v64, _ = R.run(params, m, v, grads, np.float64)
    p32, m32, v32, _ = R.run(params, m, v, grads, np.float32)
    worst = max(within(state["m"], m64, m32, "m"), within(state["v"], v64, v32, "v"))
    for k in R.GROUPS:
        if p[k].numel():
            worst = max(worst, within(p[k], p64[k], p32[k], k))
    print(f"n {n}, n_coef {n_coef}: worst measured / bound {worst:.3f}")


def test_vector_and_scalar_paths_give_the_same_bits(ops):
    """n a multiple of 4, so every m / v slice of an aligned buffer is 16-byte aligned: with aligned pointers every group takes the
    16-byte path, with every pointer 4 bytes past a boundary every group takes the 4-byte path."""
    n, n_coef = 1028, 16
    params, m, v, grads = R.random_case(n, n_coef, 5)
    out = {}
    for shift in (0, 4):
        handles, p, state = upload(params, m, v, shift)
        assert all(t.data_ptr() % 16 == shift for t in list(p.values()) + [state["m"], state["v"]])
        sl = ops.gaussian_adam_slices(n, n_coef)
        assert all((state["m"].data_ptr() + 4 * sl[k].start) % 16 == shift for k in R.GROUPS)
        for step, g in enumerate(grads):
            ops.gaussian_adam(p, upload_grads(g, shift), state, step, R.LRS, **R.HYPER)
        torch.cuda.synchronize()
        assert all(guards_intact(h) for h in handles) and int(state["status"]) == 0
        out[shift] = snapshot(p, state)
    assert same_bits(out[0], out[4])
    # a mixed case: aligned bases but n = 63, so only the slices at offset 0 are aligned and xyz ends in a partial quad
    params, m, v, grads = R.random_case(63, 4, 6)
    for shift in (0, 4):
        handles, p, state = upload(params, m, v, shift)
        for step, g in enumerate(grads):
            ops.gaussian_adam(p, upload_grads(g, shift), state, step, R.LRS, **R.HYPER)
        torch.cuda.synchronize()
        assert all(guards_intact(h) for h in handles)
        out[shift] = snapshot(p, state)
    assert same_bits(out[0], out[4])


def test_frozen_group_keeps_its_bits(ops):
    n, n_coef = 257, 4
    params, m, v, grads = R.random_case(n, n_coef, 7, steps=1)
    _, p, state = upload(params, m, v)
    before = snapshot(p, state)
    g = upload_grads(dict(grads[0], f_dc=None, rot=None))
    del g["rot"]                                                       # absent and None both freeze
    ops.gaussian_adam(p, g, state, 0, R.LRS, **R.HYPER)
    sl = ops.gaussian_adam_slices(n, n_coef)
    for k in R.GROUPS:
        same = [torch.equal(bits(p[k].reshape(-1)), bits(before[k])), torch.equal(bits(state["m"][sl[k]]), bits(before["m"][sl[k]])),
                torch.equal(bits(state["v"][sl[k]]), bits(before["v"][sl[k]]))]
        assert all(same) if k in ("f_dc", "rot") else not any(same), k
    assert int(state["status"]) == 0


def test_not_finite_entries_are_left_out(ops):
    n, n_coef = 257, 4
    params, m, v, grads = R.random_case(n, n_coef, 8, steps=1)
    plant = {k: a.copy() for k, a in grads[0].items()}
    plant["scale"][300], plant["f_rest"][2000] = np.inf, np.nan
    runs = []
    for g in (grads[0], plant):
        _, p, state = upload(params, m, v)
        start = snapshot(p, state)
        ops.gaussian_adam(p, upload_grads(g), state, 0, R.LRS, **R.HYPER)
        runs.append((snapshot(p, state), int(state["status"])))
    (clean, st0), (planted, st1) = runs
    assert st0 == 0 and st1 == R.STATUS_NOT_FINITE
    sl = ops.gaussian_adam_slices(n, n_coef)
    for k, i in (("scale", 300), ("f_rest", 2000)):
        j = sl[k].start + i
        assert planted[k][i] == start[k][i] and planted["m"][j] == start["m"][j] and planted["v"][j] == start["v"][j]
        assert clean[k][i] != start[k][i]
        clean[k][i], clean["m"][j], clean["v"][j] = start[k][i], start["m"][j], start["v"][j]
    assert same_bits(clean, planted)


def test_capacity_overflow_changes_nothing_now_or_later(ops):
    n, n_coef = 65, 4
    params, m, v, grads = R.random_case(n, n_coef, 9, steps=1)
    _, p, state = upload(params, m, v)
    g = upload_grads(grads[0])
    count = torch.tensor([100], dtype=torch.int64, device="cuda")
    ops.gaussian_adam(p, g, state, 0, R.LRS, instances=count, max_instances=100, **R.HYPER)            # fits: the step is taken
    moved = snapshot(p, state)
    assert int(state["status"]) == 0 and not torch.equal(moved["xyz"], torch.from_numpy(params["xyz"]).cuda())
    count.fill_(101)
    ops.gaussian_adam(p, g, state, 1, R.LRS, instances=count, max_instances=100, **R.HYPER)
    assert int(state["status"]) == R.STATUS_CAPACITY and same_bits(moved, snapshot(p, state))
    count.fill_(50)
    ops.gaussian_adam(p, g, state, 2, R.LRS, instances=count, max_instances=100, **R.HYPER)            # bit 1 is read on entry
    ops.gaussian_adam(p, g, state, 3, R.LRS, **R.HYPER)
    assert int(state["status"]) == R.STATUS_CAPACITY and same_bits(moved, snapshot(p, state))


def test_opacity_reset(ops):
    n, n_coef = 4099, 4
    params, m, v, _ = R.random_case(n, n_coef, 10, steps=0)
    params["opacity"] = np.linspace(-12.0, 12.0, n).astype(np.float32)
    handles, p, state = upload(params, m, v)
    before = snapshot(p, state)
    sl = ops.gaussian_adam_slices(n, n_coef)
    ops.opacity_reset(p["opacity"], state["m"][sl["opacity"]], state["v"][sl["opacity"]], ceiling=0.01)
    torch.cuda.synchronize()
    assert all(guards_intact(h) for h in handles)
    x = params["opacity"]
    within(p["opacity"], R.reset(x.astype(np.float64), 0.01, np.float64), R.reset(x, 0.01, np.float32), "reset")
    assert float(p["opacity"].max()) <= float(np.log(0.01 / 0.99)) + 1e-5
    for name in ("m", "v"):
        assert not bool(state[name][sl["opacity"]].any()) and bool(before[name][sl["opacity"]].any())
        for k in R.GROUPS:
            if k != "opacity":
                assert torch.equal(bits(state[name][sl[k]]), bits(before[name][sl[k]])), (name, k)
    assert all(torch.equal(bits(p[k].reshape(-1)), bits(before[k])) for k in R.GROUPS if k != "opacity")
    # plain opacities: min(x, ceiling); and without the optimiser's slices
    plain = torch.tensor([0.0, 0.005, 0.01, 0.5, 1.0], device="cuda")
    ops.opacity_reset(plain, ceiling=0.01, opacity_is_logit=False)
    assert plain.tolist() == [0.0, float(np.float32(0.005)), float(np.float32(0.01)), float(np.float32(0.01)), float(np.float32(0.01))]


def test_same_bytes_on_two_calls(ops):
    n, n_coef = 4099, 16
    params, m, v, grads = R.random_case(n, n_coef, 11)
    out = []
    for _ in range(2):
        _, p, state = upload(params, m, v)
        for step, g in enumerate(grads):
            ops.gaussian_adam(p, upload_grads(g), state, step, R.LRS, **R.HYPER)
        out.append(snapshot(p, state))
    assert same_bits(out[0], out[1])
