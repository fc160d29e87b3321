"""One bad (or legal) call of a temporal entry point without a GPU, by case name: what tests/test_temporal_abi.py
and tests/test_temporal_motion_abi.py share.  A helper module like temporal_cases.py."""
import numpy as np

PARAM_NAMES = ("alpha", "alpha_m", "tau_n", "tau_z", "tau_a", "eps_a", "min_history", "w_min")
GOOD = (0.2, 0.2, 0.9, 0.02, 0.05, 1e-2, 4.0, 0.25)
FAKE = 4096   # a device "pointer" that is never dereferenced: the checks fail first
MAX_OBJECTS = 1 << 20
# every parameter at each value that is illegal for it
ILLEGAL = {
    "alpha": {"neg": -0.1, "above": 1.5, "nan": np.nan, "inf": np.inf},
    "alpha_m": {"neg": -0.1, "above": 1.5, "nan": np.nan, "inf": np.inf},
    "tau_n": {"below": -1.5, "above": 1.5, "nan": np.nan, "inf": np.inf},
    "tau_z": {"0": 0.0, "neg": -1.0, "nan": np.nan, "inf": np.inf},
    "tau_a": {"neg": -1.0, "nan": np.nan, "inf": np.inf},
    "eps_a": {"0": 0.0, "neg": -1.0, "nan": np.nan, "inf": np.inf},
    "min_history": {"0": 0.0, "half": 0.5, "neg": -1.0, "nan": np.nan, "inf": np.inf},
    "w_min": {"0": 0.0, "neg": -1.0, "above": 1.5, "nan": np.nan, "inf": np.inf},
}


def cam(aperture=0.0):
    rec = np.zeros(24, np.float32)
    rec[[0, 5, 10, 15]] = 1.0
    rec[16:20] = (0.5, 0.5, 1.0, aperture)
    return rec


def call(L, N, device_form, case, motion=False):
    """(rc, error text, the entry point's name with a colon, the state plane) of prt_temporal_accumulate, or with
    `motion` prt_temporal_accumulate_motion, in the host or the device form.  The state is pre-filled with 1."""
    W, H, device, n_objects = 4, 3, 0, 2
    color = np.zeros((W, H, 3), np.float32)
    feat = np.zeros((W, H, 8), np.float32)
    state = np.ones((W, H, 8), np.float32)
    pfeat, pstate = feat.copy(), np.zeros((W, H, 8), np.float32)
    ids, pids = np.zeros((W, H), np.int32), np.zeros((W, H), np.int32)
    table = np.zeros((n_objects, 12), np.float32)
    rec, prec = cam(), cam()
    prec[3] = 0.5
    par = np.array(GOOD, np.float32)
    if device_form:
        p = dict(color=FAKE, feat=FAKE * 2, state=FAKE * 3, prev_feat=FAKE * 4, prev_state=FAKE * 5, ids=FAKE * 6,
                 prev_ids=FAKE * 7, motion=FAKE * 8)
    else:
        p = dict(color=N.ptr(color), feat=N.ptr(feat), state=N.ptr(state), prev_feat=N.ptr(pfeat),
                 prev_state=N.ptr(pstate), ids=N.ptr(ids), prev_ids=N.ptr(pids), motion=N.ptr(table))
    p.update(cam=N.ptr(rec), prev_cam=N.ptr(prec), params=N.ptr(par))
    prevs = ("prev_feat", "prev_cam", "prev_state") + (("prev_ids",) if motion else ())
    if case.startswith("null_"):
        p[{"null_params": "params"}.get(case, case[5:])] = None
    elif case.startswith("only_"):
        for k in prevs:
            if k != case[5:]:
                p[k] = None
    elif case.startswith("no_"):
        p[case[3:]] = None
    elif case == "n_neg":
        n_objects = -1
    elif case == "n_huge":
        n_objects = MAX_OBJECTS + 1
    elif case in ("w0", "w_neg", "w_huge"):
        W = {"w0": 0, "w_neg": -3, "w_huge": 32769}[case]
    elif case in ("h0", "h_huge"):
        H = {"h0": 0, "h_huge": 32769}[case]
    elif case == "device_neg":
        device = -1
    elif case == "aperture":   # the motion tests' one aperture case is the previous camera's
        (prec if motion else rec)[19] = 0.1
    elif case == "prev_aperture":
        prec[19] = 0.1
    elif case == "cam_nan":
        rec[7] = np.nan
    elif case == "prev_cam_inf":
        prec[16] = np.inf
    elif case == "tau_z":
        par[3] = 0.0
    elif ":" in case:
        name, how = case.split(":")
        par[PARAM_NAMES.index(name)] = ILLEGAL[name][how]
    elif case.startswith("legal="):
        _, name, value = case.split("=")
        par[PARAM_NAMES.index(name)] = float(value)
        device = 1 << 20
    elif case == "legal":
        device = 1 << 20
    elif case == "legal_empty":   # an empty table needs no pointer
        device, n_objects, p["motion"] = 1 << 20, 0, None
    elif case == "legal_first":   # the first frame: every prev pointer NULL
        device = 1 << 20
        for k in prevs:
            p[k] = None
    elif case == "legal_max":
        device, n_objects = 1 << 20, MAX_OBJECTS
    else:
        raise ValueError(case)
    moving = (p["ids"], p["prev_ids"], p["motion"], n_objects) if motion else ()
    args = (device, p["color"], p["feat"], p["cam"], p["prev_feat"], p["prev_cam"], p["prev_state"], *moving, W, H,
            p["params"], p["state"], None, None) + ((None,) if device_form else ())
    name = "prt_temporal_accumulate" + ("_motion" if motion else "") + ("_device" if device_form else "")
    return getattr(L, name)(*args), L.prt_denoise_last_error(), name.encode() + b":", state
