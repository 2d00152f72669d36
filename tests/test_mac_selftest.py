"""The MAC kernels' per-lane steps and CRC combine arithmetic on the CPU:
c-ofdm_amd/apps/mac_selftest.cpp runs the shared code of csrc/ofdm_mac.hpp
lane by lane against a bytewise CRC-32 for every covered length up to 4200,
built with the host's address and undefined-behaviour sanitizers."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SELFTEST = os.path.join(ROOT, "c-ofdm_amd", "bin", "mac_selftest")


def test_mac_selftest():
    subprocess.run(["make", "-C", os.path.join(ROOT, "c-ofdm_amd"), "bin/mac_selftest"], check=True,
                   capture_output=True)
    r = subprocess.run([SELFTEST], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "mac_selftest: ok" in r.stdout
