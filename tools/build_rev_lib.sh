#!/bin/bash
# A/B against an earlier commit: the library as built from REV's sources (csrc/ + include/, with
# the current build.py flags; with REV's own build.py when REV lacks one of today's translation
# units, e.g. a commit from before csrc/abi.hip) under tools/diag/NAME/libballenv.so (git-ignored), e.g.
#   bash tools/build_rev_lib.sh HEAD prev      # then BALLENV_LIB=tools/diag/prev/libballenv.so
set -eu
cd "$(dirname "$0")/.."
rev=$1; name=$2
tmp=$(mktemp -d)
mkdir -p $tmp/gym-ballenv_amd/csrc $tmp/include tools/diag/$name
git archive "$rev" gym-ballenv_amd/csrc gym-ballenv_amd/build.py include | tar -x -C $tmp
python3 - "$tmp" "$name" <<'PY'
import os, shutil, sys
sys.path.insert(0, "gym-ballenv_amd")
import build as current
rev_pkg = os.path.join(sys.argv[1], "gym-ballenv_amd")
if all(os.path.exists(os.path.join(rev_pkg, "csrc", u)) for u in current.UNITS):
    shutil.copy("gym-ballenv_amd/build.py", os.path.join(rev_pkg, "build.py"))
del sys.modules["build"]
sys.path[0] = rev_pkg
import build
build.build_library(force=True, verbose=False, out=os.path.abspath(f"tools/diag/{sys.argv[2]}/libballenv.so"))
PY
rm -rf $tmp
echo "built tools/diag/$name/libballenv.so from $rev"
