"""The stream receiver's host stitch (c-ofdm_amd/csrc/ofdm_stream_stitch.hpp)
without a GPU: c-ofdm_amd/apps/stitch_selftest.cpp runs stitch_chunks,
located_list and spec_list on hand-written walk tables of 3-4 chunks: chunks
that share a record with their predecessor, re-walks (no shared record, a
shared record past the first owned frame, equal preamble starts with
different lag bits), a walk that ends early, a frame before sample 0, record
overflow before and after a re-walk, and the located list's head/tail
truncation."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SELFTEST = os.path.join(ROOT, "c-ofdm_amd", "bin", "stitch_selftest")


def test_stitch_selftest():
    # plain host C++ (one header): built here where the tree was not built
    subprocess.run(["make", "-C", os.path.join(ROOT, "c-ofdm_amd"), "bin/stitch_selftest"], check=True,
                   capture_output=True)
    r = subprocess.run([SELFTEST], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
