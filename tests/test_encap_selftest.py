"""CPU self-test of the encapsulation rule's reads and writes
(f-stack_amd/csrc/encap.h) under the host compiler's address and
undefined-behaviour sanitizers: a stand-alone program, built and run the way
test_decap_selftest.py builds its program.  Nothing is loaded into python."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]


def test_encap_rule_touches_only_its_rooms(tmp_path):
    """Packets of every kind, every ip_hl x hlen and every refusal in heap
    blocks of exactly headroom + len + tailroom bytes, the rooms exactly what
    the packet needs (tools/encap_selftest.cpp)."""
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    r = subprocess.run(["g++"] + SAN + ["-o", str(tmp_path / "probe"), str(probe)], capture_output=True, text=True,
                       timeout=300)
    if r.returncode != 0:
        pytest.skip("the host compiler's sanitizer runtime is not installed: " + r.stderr[-200:])
    exe = tmp_path / "encap_selftest"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17"] + SAN +
                   ["-I", os.path.join(ROOT, "f-stack_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                    "-o", str(exe), os.path.join(ROOT, "tools", "encap_selftest.cpp")], check=True, timeout=300)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert r.stdout.startswith("OK")
