"""Dynamic mixing (dynamic_mix.py; ctn_dmix_draw / ctn_dmix_mix) checks that need no GPU:
the Philox generator against the Random123 known answers, the properties of the host plan,
the C entries' exports, limits and argument validation, the loader's step arithmetic, the
train.py flags and the corpus reader."""
import ctypes
import json
import os

import numpy as np
import pytest

import dynamic_mix as dm


@pytest.fixture(scope="module")
def lib():
    import ctn_lib as L
    if not os.path.exists(L.LIB_PATH):
        pytest.fail(f"{L.LIB_PATH} not built (run make / __graft_entry__.build())")
    return L.load()


# ------------------------------------------------------------------ Philox
@pytest.mark.parametrize("counter,key,want", [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
     "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_philox_known_answers(counter, key, want):
    assert " ".join(f"{w:08x}" for w in dm.philox4x32_10(counter, key)) == want


# ------------------------------------------------------------------ host plan
def _corpus(lens, spk):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64), np.asarray(spk, np.int32)


LENS = [4200, 1000, 5000, 1, 3000, 1000, 2500, 4099, 999, 1200, 1700, 4100]
SPK = [0, 0, 1, 0, 0, 2, 0, 0, 1, 0, 0, 0]


def test_plan_start_range_and_exact_length():
    off, spk = _corpus(LENS, SPK)
    T = 1000
    elig = dm.eligible(off, T)
    assert elig.tolist() == [i for i, n in enumerate(LENS) if n >= T]
    plan = dm.plan_host(off, spk, elig, 40, 2, T, seed=3)
    n = np.diff(off)[plan["utt"]]
    assert (plan["start"] >= 0).all() and (plan["start"] + T <= n).all()
    exact = n == T
    assert exact.any() and (plan["start"][exact] == 0).all()
    assert (plan["level_db"] >= -2.5).all() and (plan["level_db"] <= 2.5).all()
    assert plan["level_db"].std() > 0.5


def test_plan_speakers_distinct_unless_exhausted():
    off, spk = _corpus(LENS, SPK)
    elig = dm.eligible(off, 1000)
    plan = dm.plan_host(off, spk, elig, 60, 3, 1000, seed=1, max_tries=16)
    assert (plan["tries"] > 1).any(), "the dominant speaker must cause rejections"
    for row in plan:
        if (row["tries"] < 16).all():
            assert len(set(spk[row["utt"]].tolist())) == 3


def test_plan_exhaustion_keeps_the_last_candidate():
    off, spk = _corpus([500, 600, 700], [7, 7, 7])
    plan = dm.plan_host(off, spk, dm.eligible(off, 100), 9, 2, 100, seed=5, max_tries=4)
    assert (plan["tries"][:, 0] == 1).all() and (plan["tries"][:, 1] == 4).all()
    assert (plan["utt"] >= 0).all()


def test_plan_row_depends_on_seed_and_global_sample_only():
    off, spk = _corpus(LENS, SPK)
    elig = dm.eligible(off, 1000)
    kw = dict(C=2, T=1000, seed=11)
    whole = dm.plan_host(off, spk, elig, M=8, first_sample=40, **kw)      # world 1, M 8, step 5
    r0 = dm.plan_host(off, spk, elig, M=4, first_sample=(5 * 2 + 0) * 4, **kw)
    r1 = dm.plan_host(off, spk, elig, M=4, first_sample=(5 * 2 + 1) * 4, **kw)
    assert np.array_equal(np.concatenate([r0, r1]), whole)
    one = dm.plan_host(off, spk, elig, M=1, first_sample=43, **kw)
    assert np.array_equal(one[0], whole[3])
    assert not np.array_equal(dm.plan_host(off, spk, elig, M=8, first_sample=40, C=2, T=1000, seed=12), whole)


def test_mix_host_contract_and_invalid_row():
    rng = np.random.default_rng(0)
    pool = rng.integers(-32768, 32767, 3000).astype(np.int16)
    off = np.array([0, 1000, 3000], np.int64)
    plan = np.zeros((2, 2), dm.PLAN_DTYPE)
    plan[0] = [(0, 3, 1.5, 1), (1, 1001, -2.0, 1)]
    plan[1] = [(0, 0, 0.0, 1), (0, 902, 0.0, 1)]                     # 902 + 99 = 1001 > 1000
    r = dm.mix_host(pool, off, plan, 99, peak=0.9)
    assert r["status"].tolist() == [0, 1]
    assert not r["sources"][1].any() and not r["mixture"][1].any()
    assert r["p"][0] > 0.9 and np.abs(r["mixture"][0]).max() <= 0.9 * (1 + 1e-6)
    x0 = pool[3:102].astype(np.float32) / np.float32(32768)
    assert np.array_equal(r["sources"][0, 0], r["gains"][0, 0].astype(np.float32) * x0)
    assert np.array_equal(r["mixture"][0], r["sources"][0, 0] + r["sources"][0, 1])


# ------------------------------------------------------------------ C entries
def _desc(**kw):
    import ctn_lib as L
    d = dict(M=4, C=2, T=1000, n_utts=12, n_elig=9, pool_dtype=0, level_mode=0, max_tries=16, level_lo_db=-2.5,
             level_hi_db=2.5, peak=0.9, seed=1)
    d.update(kw)
    return L.DmixDesc(**d)


def test_symbols_and_descriptor_layout(lib):
    import ctn_lib as L
    for name in ("ctn_dmix_workspace_bytes", "ctn_dmix_draw", "ctn_dmix_mix"):
        assert name in L.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert [f[0] for f in L.DmixDesc._fields_] == ["M", "C", "T", "n_utts", "n_elig", "pool_dtype", "level_mode",
                                                  "max_tries", "level_lo_db", "level_hi_db", "peak", "seed"]
    assert ctypes.sizeof(L.DmixDesc) == 56 and L.DmixDesc.seed.offset == 48
    assert ctypes.sizeof(L.DmixEntry) == 16 == dm.PLAN_DTYPE.itemsize
    assert [f[0] for f in L.DmixEntry._fields_] == list(dm.PLAN_DTYPE.names)
    assert lib.ctn_abi_version() == 13                   # added without a version bump


def test_workspace_bytes_at_and_beyond_each_limit(lib):
    ws = lambda **kw: lib.ctn_dmix_workspace_bytes(ctypes.byref(_desc(**kw)))   # noqa: E731
    assert ws() > 0
    assert ws(M=8) > ws() and ws(T=5000) > ws()
    for ok in (dict(C=1), dict(C=16), dict(T=1), dict(n_elig=1), dict(max_tries=1), dict(max_tries=64),
               dict(pool_dtype=1, level_mode=1), dict(peak=0.0)):
        assert ws(**ok) > 0, ok
    for bad in (dict(C=0), dict(C=17), dict(T=0), dict(n_elig=0), dict(max_tries=0), dict(max_tries=65),
                dict(M=0), dict(n_utts=0), dict(pool_dtype=2), dict(level_mode=-1), dict(peak=-1.0),
                dict(peak=float("nan")), dict(level_lo_db=float("inf"))):
        assert ws(**bad) == 0, bad
    assert lib.ctn_dmix_workspace_bytes(None) == 0


def test_entries_validate_before_the_device(lib):
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    d = _desc()
    assert lib.ctn_dmix_draw(None, p, p, p, 0, None, 0, p, None) == 1
    assert lib.ctn_dmix_mix(None, p, p, p, p, p, p, p, p, 64, None) == 1
    for i in range(4):                                   # off, spk, elig, plan
        a = [p, p, p, 0, None, 0, p]
        a[i if i < 3 else 6] = None
        assert lib.ctn_dmix_draw(ctypes.byref(d), *a, None) == 1
        assert "null pointer" in lib.ctn_last_error().decode()
    for i in range(7):                                   # pool, off, plan, gains, sources, mixture, status
        a = [p] * 7
        a[i] = None
        assert lib.ctn_dmix_mix(ctypes.byref(d), *a, p, 1 << 30, None) == 1
        assert "null pointer" in lib.ctn_last_error().decode()
    for bad, rc in ((dict(C=0), 1), (dict(T=0), 1), (dict(n_elig=0), 1), (dict(max_tries=0), 1),
                    (dict(C=17), 2), (dict(max_tries=65), 2)):
        b = _desc(**bad)
        assert lib.ctn_dmix_draw(ctypes.byref(b), p, p, p, 0, None, 0, p, None) == rc, bad
        assert lib.ctn_last_error().decode()
        assert lib.ctn_dmix_mix(ctypes.byref(b), p, p, p, p, p, p, p, p, 1 << 30, None) == rc, bad
    assert lib.ctn_dmix_mix(ctypes.byref(d), p, p, p, p, p, p, p, None, 0, None) == 3      # no workspace
    assert lib.ctn_dmix_mix(ctypes.byref(d), p, p, p, p, p, p, p, p, 8, None) == 3         # short workspace
    assert "workspace" in lib.ctn_last_error().decode()
    assert lib.ctn_dmix_mix(ctypes.byref(d), p + 1, p, p, p, p, p, p, p, 1 << 30, None) == 1
    assert "aligned" in lib.ctn_last_error().decode()


# ------------------------------------------------------------------ Python surface
def test_train_parser_defaults_and_cpu_refusal():
    import train
    a = train.parser.parse_args([])
    assert a.dynamic_mix == 0 and a.dm_seed == 0 and a.dm_level_mode == 0 and a.dm_steps == 0
    assert a.dm_level_db == [-2.5, 2.5] and a.dm_peak == 0.9
    a = train.parser.parse_args(["--dynamic_mix", "1", "--dm_level_db", "-5", "0", "--dm_steps", "7", "--use_cuda", "0"])
    assert a.dynamic_mix == 1 and a.dm_level_db == [-5.0, 0.0] and a.dm_steps == 7
    with pytest.raises(ValueError, match="use_cuda"):
        train.main(a)


class _FakeMixer:
    def batch(self, step):
        return step


def test_loader_len_epoch_and_steps():
    ld = dm.DynamicMixLoader(_FakeMixer(), 3)
    assert len(ld) == 3 and ld.sampler is ld
    assert list(ld) == [0, 1, 2]
    ld.sampler.set_epoch(4)                              # what Solver._run_one_epoch calls
    assert list(ld) == [12, 13, 14] and list(ld) == [12, 13, 14]
    with pytest.raises(ValueError):
        dm.DynamicMixLoader(_FakeMixer(), 0)


def test_wsj0_speaker_rule():
    name = "/x/011a0101_1.8_40na010x_-1.8.wav"
    assert dm.wsj0_speaker_of(name, 1) == "011" and dm.wsj0_speaker_of(name, 2) == "40n"
    assert dm.wsj0_speaker_of("/x/a.wav", 1) != dm.wsj0_speaker_of("/x/b.wav", 1)
    assert dm.wsj0_speaker_of("/x/011a0101_1.8.wav", 2) == ("file", "/x/011a0101_1.8.wav", 2)


def test_from_json_dir_reads_pcm16(tmp_path):
    import audio_io
    rng = np.random.default_rng(2)
    names = {"s1": ["011a_0_40na_0.wav", "012b_0_40nb_0.wav"], "s2": ["011a_0_40na_0.wav"]}
    waves = {}
    for s, files in names.items():
        os.makedirs(tmp_path / s)
        infos = []
        for i, f in enumerate(files):
            x = rng.uniform(-1, 1, 50 + 7 * i + len(s) * len(waves))
            path = str(tmp_path / s / f)
            audio_io.write_wav(path, x, 8000)
            waves[path] = audio_io.read_wav(path)[0]
            infos.append([path, len(x)])
        with open(tmp_path / f"{s}.json", "w") as fh:
            json.dump(infos, fh)
    c = dm.DeviceCorpus.from_json_dir(str(tmp_path), 8000, device="cpu")
    assert c.pool_dtype == 0 and c.pool.dtype.is_floating_point is False and c.n_utts == 3
    assert c.spk_host.tolist() == [0, 1, 2] and c.speaker_labels == ["011", "012", "40n"]
    pool = c.pool.numpy()
    for i, x in enumerate(waves.values()):               # exactly what read_wav returns
        seg = pool[c.off_host[i]:c.off_host[i + 1]]
        assert np.array_equal(seg.astype(np.float32) * np.float32(2.0 ** -15), x)
    assert c.nbytes == 2 * len(pool) + 8 * 4 + 4 * 3
    assert c.eligible(50, 3)[1].tolist() == [0, 1, 2]
    with pytest.raises(ValueError, match="distinct speakers"):
        c.eligible(57, 3)                                # only one utterance is that long
    with pytest.raises(ValueError, match="max_bytes"):
        dm.DeviceCorpus.from_json_dir(str(tmp_path), 8000, max_bytes=100, device="cpu")
    same = dm.DeviceCorpus.from_json_dir(str(tmp_path), 8000, speaker_of=lambda p, s: "x", device="cpu")
    with pytest.raises(ValueError, match="distinct speakers"):
        same.eligible(10, 2)
    fp = dm.DeviceCorpus([np.zeros(4, np.int16), np.ones(3, np.float32)], ["a", "b"], "cpu")
    assert fp.pool_dtype == 1 and fp.pool.dtype.is_floating_point
