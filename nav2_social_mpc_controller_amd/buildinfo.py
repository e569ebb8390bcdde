"""Identity of the device sources a number was measured on.

The GPU box receives the tree without `.git`, so `git rev-parse HEAD:nav2_social_mpc_controller_amd/csrc` is not
available where profiles are taken. `csrc_digest()` is its stand-in: a SHA-256 over the kernel sources and the build
recipe (names and contents, sorted). Profile summaries under `profiles/` record it; `bench.py` only uses instruction
counts from a summary whose digest equals that of the sources it is running on."""
import hashlib
import os

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc")
SOURCE_SUFFIXES = (".hpp", ".hip", ".inc", ".h", ".sh")


def csrc_digest(root: str = CSRC) -> str:
    h = hashlib.sha256()
    names = sorted(f for f in os.listdir(root) if f.endswith(SOURCE_SUFFIXES))
    extra = os.path.join(os.path.dirname(os.path.dirname(root)), "include", "smpc.h")
    for path in [os.path.join(root, n) for n in names] + ([extra] if os.path.exists(extra) else []):
        h.update(os.path.basename(path).encode() + b"\0")
        with open(path, "rb") as f:
            h.update(f.read())
        h.update(b"\0")
    return h.hexdigest()[:16]


if __name__ == "__main__":
    print(csrc_digest())
