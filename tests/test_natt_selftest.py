"""CPU self-test of the NAT-T rules' reads and writes (f-stack_amd/csrc:
classify.h, decap.h, encap.h, natt.h) under the host compiler's address and
undefined-behaviour sanitizers: a stand-alone program, built and run the way
test_decap_selftest.py builds its program.  Nothing is loaded into python."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]


def test_natt_rules_touch_only_the_packet(tmp_path):
    """UDP-encapsulated packets for classification, the header moves of both
    directions over every ip_hl x hlen, and the checksum fix over every
    segment length 0..530 and 65515, each in an exact-size heap block
    (tools/natt_selftest.cpp)."""
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    r = subprocess.run(["g++"] + SAN + ["-o", str(tmp_path / "probe"), str(probe)], capture_output=True, text=True,
                       timeout=300)
    if r.returncode != 0:
        pytest.skip("the host compiler's sanitizer runtime is not installed: " + r.stderr[-200:])
    exe = tmp_path / "natt_selftest"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17"] + SAN +
                   ["-I", os.path.join(ROOT, "f-stack_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                    "-o", str(exe), os.path.join(ROOT, "tools", "natt_selftest.cpp")], check=True, timeout=300)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert r.stdout.startswith("OK")
