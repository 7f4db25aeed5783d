"""CPU self-test of the outbound AH rules' reads and writes (f-stack_amd/csrc:
ah_out.h) under the host compiler's address and undefined-behaviour
sanitizers: a stand-alone program, built and run the way
test_ah_in_selftest.py builds its program.  Nothing is loaded into python."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]


def test_ah_out_rules_touch_only_the_headroom_the_packet_and_the_slot(tmp_path):
    """The three rules over every ip_hl 5..15 x mlen {12, 16, 24, 32} x family
    of packet and SA x mode, headroom and packet in one exact-size heap block
    and the save slot in another; headroom one byte short; the option loop's
    refusals at the last byte of the header and the short source routes
    (tools/ah_out_selftest.cpp)."""
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    r = subprocess.run(["g++"] + SAN + ["-o", str(tmp_path / "probe"), str(probe)], capture_output=True, text=True,
                       timeout=300)
    if r.returncode != 0:
        pytest.skip("the host compiler's sanitizer runtime is not installed: " + r.stderr[-200:])
    exe = tmp_path / "ah_out_selftest"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17"] + SAN +
                   ["-I", os.path.join(ROOT, "f-stack_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                    "-o", str(exe), os.path.join(ROOT, "tools", "ah_out_selftest.cpp")], check=True, timeout=300)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert r.stdout.startswith("OK")
