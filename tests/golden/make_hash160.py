"""Writes tests/golden/hash160_vectors.json: 32-byte keys with their RIPEMD-160
and Hash160 = RIPEMD160(SHA256(key)) (HashUtilities.cpp:22-29) computed by
OpenSSL, the library the reference calls, plus RIPEMD-160's published test
messages digested the same way.

  python tests/golden/make_hash160.py

Needs an `openssl` whose legacy provider has RIPEMD-160; fails if it has not
(no fallback: the file's worth is that OpenSSL made it).  The tests read the
JSON only.
"""
import hashlib
import json
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OPENSSL = ["openssl", "dgst", "-ripemd160", "-provider", "legacy", "-provider", "default", "-binary"]

# the messages of the RIPEMD-160 publication's test set (the million-'a' one left out)
MESSAGES = ["", "a", "abc", "message digest", "abcdefghijklmnopqrstuvwxyz",
            "abcdbcdecdefdefgefghfghighijhijkijkljklmklmnlmnomnopnopq",
            "ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789", "1234567890" * 8]


def openssl_ripemd160(data):
    r = subprocess.run(OPENSSL, input=bytes(data), capture_output=True, check=True)
    if len(r.stdout) != 20:
        raise RuntimeError("openssl has no RIPEMD-160: " + r.stderr.decode(errors="replace"))
    return r.stdout


def keys():
    out = [bytes(32), b"\xff" * 32]
    for bit in range(256):
        k = bytearray(32)
        k[bit >> 3] = 1 << (bit & 7)
        out.append(bytes(k))
    g = np.load(os.path.join(HERE, "ed25519_golden.npz"), allow_pickle=False)
    seen = set(out)
    for row in g["pk"]:
        k = row.tobytes()
        if k not in seen:
            seen.add(k)
            out.append(k)
    rng = np.random.default_rng(0x160)
    out += [rng.bytes(32) for _ in range(64)]
    return out


def main():
    version = subprocess.run(["openssl", "version"], capture_output=True, text=True, check=True).stdout.strip()
    assert openssl_ripemd160(b"abc").hex() == "8eb208f7e05d987a9b044a8e98c6b087f15a0bfc"
    ks = keys()
    doc = {
        "source": "openssl dgst -ripemd160 -provider legacy -provider default; SHA-256 by hashlib (the same OpenSSL)",
        "openssl_version": version,
        "messages": [{"ascii": m, "ripemd160": openssl_ripemd160(m.encode()).hex()} for m in MESSAGES],
        "keys": [k.hex() for k in ks],
        "ripemd160": [openssl_ripemd160(k).hex() for k in ks],
        "hash160": [openssl_ripemd160(hashlib.sha256(k).digest()).hex() for k in ks],
    }
    with open(os.path.join(HERE, "hash160_vectors.json"), "w") as f:
        json.dump(doc, f, indent=0)
        f.write("\n")
    print(len(ks), "keys")


if __name__ == "__main__":
    main()
