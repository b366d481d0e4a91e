# development: one-unit build of qp_solver.hip for a single tile count (default T = 5) through the checked pipeline, linked with the
# shipped objects of everything else (the Makefile's lists) -> fsae-mpc_amd/lib/libfsaempc_exp.so, or libfsaempc_$EXP_NAME.so
# (FSAEMPC_LIB selects it).  usage: [EXP_NAME=name] tools/build_exp.sh [T] [extra flags]
set -e
T=${1:-5}; shift || true
cd "$(dirname "$0")/.."
make exp EXP_T=$T EXP_NAME=${EXP_NAME:-exp} EXP_FLAGS="$*"
