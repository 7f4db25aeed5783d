#!/usr/bin/env python3
"""Extract the AH golden packets from the reference tree, as data.

Run where the reference tree is (never on a GPU host): it reads DPDK's own
known-answer vectors as text and writes tests/golden/ah_packets.json:

  pkt_ah_tunnel_sha256, pkt_ah_transport_sha256
      dpdk/app/test/test_cryptodev_security_ipsec_test_vectors.h:2241-2449
      (HMAC-SHA2-256-128: auth key, input packet, AH output packet)

The JSON holds only inputs and expected outputs (hex strings); no reference
source text is stored.  Usage:  python tests/golden/make_golden_ah.py
"""
import json
import os
import re

REF = os.environ.get("FSTACK_REF", "/root/reference")
VEC = os.path.join(REF, "dpdk", "app", "test", "test_cryptodev_security_ipsec_test_vectors.h")
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "ah_packets.json")
NAMES = ("pkt_ah_tunnel_sha256", "pkt_ah_transport_sha256")


def block(src, pos):
    """src[pos] == '{' -> the text between it and its matching '}'."""
    depth = 0
    for i in range(pos, len(src)):
        if src[i] == "{":
            depth += 1
        elif src[i] == "}":
            depth -= 1
            if depth == 0:
                return src[pos + 1:i]
    raise ValueError("unbalanced braces")


def data_of(body, field):
    """The bytes of `.field = { .data = { 0x.., ... } }` inside body."""
    m = re.search(r"\.%s\s*=\s*\{" % field, body)
    inner = block(body, m.end() - 1)
    d = re.search(r"\.data\s*=\s*\{", inner)
    return bytes(int(x, 16) for x in re.findall(r"0x[0-9a-fA-F]{1,2}", block(inner, d.end() - 1)))


def main():
    src = re.sub(r"/\*.*?\*/", " ", open(VEC).read(), flags=re.S)
    out = []
    for name in NAMES:
        m = re.search(r"struct ipsec_test_data %s\s*=\s*\{" % name, src)
        body = block(src, m.end() - 1)
        out.append({"name": name, "auth": "hmac-sha2-256-128",
                    "key": data_of(body, "auth_key").hex(),
                    "input": data_of(body, "input_text").hex(),
                    "output": data_of(body, "output_text").hex()})
    with open(OUT, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote %s (%d packets)" % (OUT, len(out)))


if __name__ == "__main__":
    main()
