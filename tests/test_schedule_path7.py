"""CPU checks of decimator path 7, "FC wherever a form exists" (csrc/zfft_schedule.cpp; no GPU
needed): zoom 2 runs fc2, zoom 4 / 8 what path 6 runs, zoom >= 16 the FC head and FC tails
("fc8+fc") while the head's output has >= 16384 samples; outside FC's domain path 7 is path 6.
The automatic choice and paths 1 .. 6 (tests/test_schedule.py TABLE) do not change.
tests/host/schedule_sweep_path7.cpp sweeps path 7 over the chooser's domain under ASan + UBSan
as a stand-alone program."""
import os
import shutil
import subprocess

from test_schedule import ROOT, TABLE, ZFFT_EUNSUPPORTED, schedule

TABLE7 = [
    # zoom 2: FC from 16384 samples, <= 65535 frames, < 2^31 bytes
    (2, 0, 7, 32768, 8, "fc2"), (2, 0, 7, 8192, 8, "unsupported"), (2, 0, 7, 16383, 1, "unsupported"),
    (2, 0, 7, 16384, 1, "fc2"), (2, 0, 7, 16384, 65535, "fc2"), (2, 0, 7, 16384, 65536, "unsupported"),
    (2, 0, 7, 299008, 4096, "fc2"), (2, 0, 7, 268435455, 1, "fc2"), (2, 0, 7, 268435456, 1, "pc2_tiles"),
    (2, 2, 7, 1073741823, 1, "fc2"), (2, 2, 7, 1073741824, 1, "pc2_tiles"), (2, 1, 7, 536870912, 1, "pc2_tiles"),
    (2, 3, 7, 536870911, 1, "fc2"),
    # zoom >= 16: the FC head, FC tails while the head's output has >= 16384 samples
    (16, 0, 7, 262144, 8, "fc8+fc"), (16, 0, 7, 16384, 1, "fc8+pc2_exact"), (64, 0, 7, 1048576, 8, "fc8+fc"),
    (16, 0, 7, 131072, 1, "fc8+fc"), (16, 0, 7, 131064, 1, "fc8+pc2_exact"), (16, 0, 7, 131064, 512, "fc8+xa"),
    (16, 0, 7, 131065, 512, "fc8+fc"), (512, 0, 7, 299008, 4096, "fc8+fc"), (16, 0, 7, 8192, 8, "unsupported"),
    (16, 0, 7, 16384, 65536, "unsupported"), (16, 0, 7, 268435456, 1, "walk8+pc2_exact"),
]
# path 7 = path 6 at these (zoom 4 / 8 everywhere; zoom 2 past FC's byte limit)
SAME_AS_6 = [(2, 0, 1 << 30, 1)] + [(z, dt, L, F) for z in (4, 8) for dt in (0, 2)
                                    for L in (8192, 16384, 32768, 299008, 268435455, 268435456, 1073741824)
                                    for F in (1, 8, 512, 65535, 65536)]


def _check(rows):
    wrong = []
    for zoom, dt, path, L, frames, want in rows:
        rc, name = schedule(zoom, dt, path, L, frames)
        if name != want or rc != (ZFFT_EUNSUPPORTED if want == "unsupported" else 0):
            wrong.append(((zoom, dt, path, L, frames), want, name, rc))
    assert not wrong, wrong


def test_schedule_table_path7():
    assert len(set(TABLE7)) == len({t[:5] for t in TABLE7})
    _check(TABLE7)


def test_path7_is_path6_where_it_adds_no_form():
    for zoom, dt, L, F in SAME_AS_6:
        assert schedule(zoom, dt, 7, L, F) == schedule(zoom, dt, 6, L, F), (zoom, dt, L, F)


def test_paths_0_to_6_unchanged():
    """Every pinned row of tests/test_schedule.py, one by one."""
    assert all(t[2] <= 6 for t in TABLE)
    for row in TABLE:
        _check([row])


def test_schedule_sweep_path7_sanitized(tmp_path):
    """Path 7 over the chooser's whole domain as a stand-alone g++ program (no HIP, no Python in
    the child) under AddressSanitizer + UBSan: tests/host/schedule_sweep_path7.cpp."""
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build tests/host/schedule_sweep_path7.cpp"
    csrc = os.path.join(ROOT, "pypanadapter_amd", "csrc")
    exe = str(tmp_path / "schedule_sweep_path7")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                    "-I", csrc, "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "host", "schedule_sweep_path7.cpp"),
                    os.path.join(csrc, "zfft_schedule.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "schedule_sweep_path7: ok" in r.stdout, r.stdout
