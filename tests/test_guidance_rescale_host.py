"""Guidance rescale (Lin et al. 2024, section 3.4) without a GPU: the float64 definition of guidance.py against the usual
formulation, the fp32 twin against the definition, the degenerate rows, the argument checks and the keywords.

Bounds.  The definition takes the ratio of standard deviations from the moments S1 = sum x, S2 = sum x^2 in float64; against
`torch.std` in float64 on a row whose mean is 4 sigma the cancellation S2 - S1^2 / n costs about 17 n^(1/2) 2^-53 relative, far
below the 1e-10 asked.  The fp32 factor f = fl(fl(phi r32) + fl(1 - phi)) against the float64 factor phi r + (1 - phi): r32 is
r rounded once (2^-24 relative), then one rounding of each of the three operations on terms that are all positive and no larger
than the sum, so at most 3 2^-24 relative plus second-order terms; 4 2^-24 is asserted."""
import importlib
import importlib.util
import inspect
import os

import numpy as np
import pytest
import torch

M = importlib.import_module("cv-diffusion-model_amd")
G = importlib.import_module("cv-diffusion-model_amd.guidance")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
EPS = 2.0 ** -24
NS = [2, 7, 1024, 1025, 12288]
WS = [-1.0, 2.5, 7.5]
PHIS = [0.25, 0.7, 1.0]


def rows(n, shift, seed=5):
    """(o_c, o_u) fp32 [3, n]: 3 N(0, 1), moved by `shift` standard deviations."""
    rng = np.random.default_rng(seed + n)
    c = (3.0 * rng.standard_normal((3, n)) + 3.0 * shift).astype(F)
    u = (3.0 * rng.standard_normal((3, n)) + 3.0 * shift).astype(F)
    return c, u


def usual_formulation(c, u, w, phi):
    """The formulation people come from, in float64 with torch.std over dims 1..: g std_c / std_g, then the phi-blend.  g is the
    fp32 guided output (the definition's), phi its fp32 value."""
    g = torch.from_numpy(G.guide_array(c, u, w).astype(np.float64))
    c64 = torch.from_numpy(c.astype(np.float64))
    dims = list(range(1, c64.dim()))
    std_c, std_g = c64.std(dim=dims, keepdim=True), g.std(dim=dims, keepdim=True)
    p = float(F(phi))
    rescaled = g * (std_c / std_g)
    out = p * rescaled + (1.0 - p) * g
    factor = p * (std_c / std_g) + (1.0 - p)
    return out.numpy(), factor.reshape(-1).numpy()


@pytest.mark.parametrize("shift", [0.0, 4.0])
@pytest.mark.parametrize("n", NS)
def test_host_definition_against_the_usual_formulation(n, shift):
    c, u = rows(n, shift)
    for w in WS:
        for phi in PHIS:
            out, factor = G.guide_rescale_host(c, u, w, phi)
            assert out.dtype == np.float64 and factor.dtype == np.float64 and out.shape == c.shape and factor.shape == (3,)
            want, want_f = usual_formulation(c, u, w, phi)
            rel_f = np.abs(factor - want_f) / np.abs(want_f)
            assert rel_f.max() <= 1e-10, (n, shift, w, phi, rel_f.max())
            scale = np.abs(want).max(axis=1, keepdims=True)
            assert (np.abs(out - want) <= 1e-10 * scale).all(), (n, shift, w, phi)


@pytest.mark.parametrize("shift", [0.0, 4.0])
@pytest.mark.parametrize("n", NS + [16389])
def test_twin_factor_and_output(n, shift):
    c, u = rows(n, shift)
    wrows = np.array([3.0, -0.5, 12.25], dtype=F)
    for w in WS + [wrows]:
        for phi in PHIS:
            _, f64 = G.guide_rescale_host(c, u, w, phi)
            # f_b as defined: the float64 ratio rounded once, then three fp32 operations
            r32 = G._rescale_ratio(c, G.guide_array(c, u, w)).astype(F)
            p = F(phi)
            fb = ((p * r32).astype(F) + F(F(1) - p)).astype(F)
            rel = np.abs(fb.astype(np.float64) - f64) / np.abs(f64)
            assert rel.max() <= 4 * EPS, (n, shift, phi, rel.max() / EPS)
            out = G.guide_rescale_array(c, u, w, phi)
            assert out.dtype == np.float32 and out.shape == c.shape
            want = (fb.reshape(-1, 1) * G.guide_array(c, u, w)).astype(F)
            assert np.array_equal(out.view(np.uint32), want.view(np.uint32))
            # the supplied factor is used as it is
            other = np.array([0.5, 1.0, 0.8125], dtype=F)
            got = G.guide_rescale_array(c, u, w, phi, factor=other)
            assert np.array_equal(got.view(np.uint32), (other.reshape(-1, 1) * G.guide_array(c, u, w)).astype(F).view(np.uint32))


def test_phi_zero_is_guide_array():
    c, u = rows(1025, 4.0)
    for w in WS:
        got = G.guide_rescale_array(c, u, w, 0.0)
        assert np.array_equal(got.view(np.uint32), G.guide_array(c, u, w).view(np.uint32))
        out, factor = G.guide_rescale_host(c, u, w, 0.0)
        assert np.array_equal(factor, np.ones(3)) and np.array_equal(out, G.guide_array(c, u, w).astype(np.float64))
        assert np.array_equal(G.guide_rescale_array(c, u, w, None).view(np.uint32), got.view(np.uint32))


def test_constant_row_and_single_element_give_factor_one():
    # short mantissas: every moment is exact in float64, so var_g is exactly 0
    c = np.full((3, 1000), 1.5, dtype=F)
    u = np.full((3, 1000), 0.25, dtype=F)
    c[1] = rows(1000, 0.0)[0][1]
    u[1] = rows(1000, 0.0)[1][1]
    for phi in PHIS:
        out, factor = G.guide_rescale_host(c, u, 2.5, phi)
        assert factor[0] == 1.0 and factor[2] == 1.0 and factor[1] != 1.0
        got = G.guide_rescale_array(c, u, 2.5, phi)
        g = G.guide_array(c, u, 2.5)
        assert np.array_equal(got[[0, 2]].view(np.uint32), g[[0, 2]].view(np.uint32)) and np.isfinite(got).all()
    c1, u1 = rows(2, 0.0)
    c1, u1 = c1[:, :1].copy(), u1[:, :1].copy()
    for phi in PHIS:
        out, factor = G.guide_rescale_host(c1, u1, 7.5, phi)
        assert np.array_equal(factor, np.ones(3)) and np.isfinite(out).all()
        assert np.array_equal(G.guide_rescale_array(c1, u1, 7.5, phi).view(np.uint32), G.guide_array(c1, u1, 7.5).view(np.uint32))


@pytest.mark.parametrize("n", [7, 1025, 12288])
def test_phi_one_matches_the_conditional_std(n):
    c, u = rows(n, 4.0)
    c4, u4 = c.reshape(3, 1, 1, n), u.reshape(3, 1, 1, n)  # trailing dims are one row
    for w in WS:
        out, _ = G.guide_rescale_host(c4, u4, w, 1.0)
        std_o, std_c = out.reshape(3, -1).std(axis=1), c.astype(np.float64).std(axis=1)
        assert (np.abs(std_o - std_c) <= 1e-6 * std_c).all()
        # the fp32 twin: one more rounding per element and the factor's
        got = G.guide_rescale_array(c4, u4, w, 1.0).astype(np.float64).reshape(3, -1).std(axis=1)
        assert (np.abs(got - std_c) <= 1e-6 * std_c).all()


def test_argument_checks():
    for bad in (True, False, float("nan"), -0.1, 1.1, "0.5", float("inf")):
        with pytest.raises(ValueError):
            G.check_guidance_rescale(bad)
    assert G.check_guidance_rescale(None) == 0.0
    for ok in (0, 0.0, 0.7, 1, 1.0, np.float32(0.25)):
        got = G.check_guidance_rescale(ok)
        assert isinstance(got, float) and got == float(ok)
    assert G.guided_keyword(2.5) == {"guidance_scale": 2.5}
    assert G.guided_keyword(None) == {}
    assert G.guided_keyword(2.5, None) == {"guidance_scale": 2.5}
    assert G.guided_keyword(2.5, 0.7) == {"guidance_scale": 2.5, "guidance_rescale": 0.7}
    assert G.guided_keyword(None, 0.7) == {"guidance_rescale": 0.7}
    with pytest.raises(ValueError):
        G.guided_keyword(2.5, 1.5)
    c = np.zeros((2, 4), dtype=F)
    for fn in (G.guide_rescale_host, G.guide_rescale_array):
        with pytest.raises(ValueError):
            fn(c, c, 2.0, 1.5)
        with pytest.raises(ValueError):
            fn(c, c, float("nan"), 0.5)
        with pytest.raises(ValueError):
            fn(c, np.zeros((2, 5), dtype=F), 2.0, 0.5)
    with pytest.raises(ValueError):
        G.guide_rescale_array(c, c, 2.0, 0.5, factor=np.ones(3, dtype=F))


def test_names_and_keywords():
    for name in ("check_guidance_rescale", "guided_keyword", "guide_rescale_host", "guide_rescale_array", "guide_rescale_device"):
        assert name in M.__all__ and getattr(M, name) is getattr(G, name), name
    kw = inspect.Parameter.KEYWORD_ONLY
    for fn in (M.LowLightDiffusion.enhance, M.LowLightDiffusion.enhance_frame, M.enhance_frame_u8, M.enhance_tiled, M.evaluate,
               M.evaluate_full_resolution):
        p = inspect.signature(fn).parameters["guidance_rescale"]
        assert (p.default, p.kind) == (None, kw), fn
    for fn in (M.LowLightTrainer.__init__, M.train_model):
        p = inspect.signature(fn).parameters["val_guidance_rescale"]
        assert (p.default, p.kind) == (None, kw), fn
    p = inspect.signature(M.LowLightLCMDistillation.__init__).parameters["guidance_rescale"]
    assert (p.default, p.kind) == (0.0, kw)
    assert inspect.signature(G.guided_enhance_host).parameters["rescale"].default is None


def toy_unet(lat, cond, t):
    return (0.3 * lat + 0.5 * cond * np.cos(lat) + 0.001 * t).astype(F)


@pytest.mark.parametrize("ptype", ["epsilon", "v_prediction"])
def test_guided_host_loop_with_rescale(ptype):
    s = M.LCMScheduler(num_train_timesteps=1000, beta_schedule="scaled_linear", prediction_type=ptype, rescale_betas_zero_snr=True)
    s.set_timesteps(4)
    ts = list(s._timestep_list)
    coefs = [s.step_coefficients(t) for t in ts]
    rng = np.random.default_rng(11)
    low = (rng.random((2, 3, 8, 8)) * 0.6 - 1.0).astype(F)
    noise = rng.standard_normal((4, 2, 3, 8, 8)).astype(F)
    # rescale=None and 0: the loop as it is without the keyword, written out
    for off in (None, 0.0):
        got = G.guided_enhance_host(toy_unet, low, noise, ts, coefs, 2.5, rescale=off)
        x = noise[0]
        for i, (t, c) in enumerate(zip(ts, coefs)):
            out = G.guide_array(toy_unet(x, low, t), toy_unet(x, np.zeros_like(low), t), 2.5)
            assert np.array_equal(got["noise_pred"][i], out)
            x = G.scheduler_step_array(out, x, noise[i + 1] if not c.is_last else None, c)
            assert np.array_equal(got["intermediate"][i], x)
        assert np.array_equal(got["enhanced"], np.clip(x, -1, 1))
    plain = G.guided_enhance_host(toy_unet, low, noise, ts, coefs, None, rescale=0.7)  # unguided: no combination, no rescale
    same = G.guided_enhance_host(toy_unet, low, noise, ts, coefs, None)
    assert all(np.array_equal(a, b) for a, b in zip(plain["intermediate"], same["intermediate"]))
    # rescale = 0.7: guide_rescale_array at every step
    got = G.guided_enhance_host(toy_unet, low, noise, ts, coefs, 2.5, rescale=0.7)
    x = noise[0]
    for i, (t, c) in enumerate(zip(ts, coefs)):
        out = G.guide_rescale_array(toy_unet(x, low, t), toy_unet(x, np.zeros_like(low), t), 2.5, 0.7)
        assert np.array_equal(got["noise_pred"][i], out)
        x = G.scheduler_step_array(out, x, noise[i + 1] if not c.is_last else None, c)
        assert np.array_equal(got["intermediate"][i], x)
    off = G.guided_enhance_host(toy_unet, low, noise, ts, coefs, 2.5)
    assert not np.array_equal(got["enhanced"], off["enhanced"])
    with pytest.raises(ValueError):
        G.guided_enhance_host(toy_unet, low, noise, ts, coefs, 2.5, rescale=1.5)


def script(name):
    spec = importlib.util.spec_from_file_location(f"_rescale_{name}", os.path.join(ROOT, "scripts", f"{name}.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_cli_flags(capsys):
    inference, train, distill, evaluate = script("inference"), script("train"), script("distill"), script("evaluate")
    a = inference.parse_args(["--input", "x.png", "--output", "y.png", "--guidance_scale", "2.5", "--guidance_rescale", "0.7"])
    assert inference.guided(a) == {"guidance_scale": 2.5, "guidance_rescale": 0.7}
    a = inference.parse_args(["--input", "x.png", "--output", "y.png", "--guidance_scale", "2.5"])
    assert a.guidance_rescale is None and inference.guided(a) == {"guidance_scale": 2.5}
    a = train.parse_args(["--guidance_scale", "3", "--guidance_rescale", "0.5"])
    assert train.guidance_from_args(a) == {"cond_dropout": 0.0, "val_guidance_scale": 3.0, "val_guidance_rescale": 0.5}
    a = distill.parse_args(["--teacher", "t.pt", "--guidance_scale_range", "4", "4", "--guidance_rescale", "0.7"])
    assert distill.guidance_keywords(a) == {"guidance_scale_range": (4.0, 4.0), "guidance": True, "guidance_rescale": 0.7}
    a = distill.parse_args(["--teacher", "t.pt", "--guidance_scale_range", "4", "4"])
    assert distill.guidance_keywords(a) == {"guidance_scale_range": (4.0, 4.0), "guidance": True}
    for mod, argv in ((inference, ["--input", "x.png", "--output", "y.png", "--guidance_rescale", "1.5"]), (train, ["--guidance_rescale", "nan"]),
                      (distill, ["--teacher", "t.pt", "--guidance_rescale", "0.7"]), (distill, ["--teacher", "t.pt", "--guidance_scale_range", "4", "4", "--guidance_rescale", "-0.1"])):
        with pytest.raises(SystemExit):
            mod.parse_args(argv)
    capsys.readouterr()
    for mod in (inference, train, distill, evaluate):
        with pytest.raises(SystemExit):
            mod.parse_args(["--help"])
        assert "--guidance_rescale" in capsys.readouterr().out, mod.__name__
