"""The host logic that the IBD entry points of the C ABI share (ngsf-hmm_amd/csrc/
capi_chain_host.hpp): the scratch carver, the cut of regions at a shard's boundaries against a
site-by-site labelling, the checks of tract records and their messages, the merge of the shards'
parts.  tests/stub/chain_host_main.cpp holds the checks; it is built as a program of its own with
the address and undefined-behaviour sanitizers, which judge every write into a carved buffer."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_chain_host_logic(tmp_path):
    exe = str(tmp_path / "chain_host_main")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan",   # the runtimes inside the program itself
                    "-I" + os.path.join(ROOT, "ngsf-hmm_amd", "csrc"),
                    os.path.join(ROOT, "tests", "stub", "chain_host_main.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout + r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all checks hold" in r.stdout
