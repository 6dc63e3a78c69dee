# Builds an A/B variant of libbeatrice_gpu.so into beatrice_amd/ab/<name>/:
#   bash tools/build_ab.sh NAME "<hipcc flags for bt_kernels.hip>" ["<g++ flags for bt_ring.cpp>"]
# Every other object comes from beatrice_amd/csrc/obj (make -C beatrice_amd/csrc first); which
# objects make the library is the Makefile's list (its print-objs target). Load the variant with
# BT_LIB_PATH (Python) or LD_LIBRARY_PATH (the C++ tools).
set -e
NAME=$1; FLAGS=$2; RING_FLAGS=$3
D=beatrice_amd/ab/$NAME
C=beatrice_amd/csrc
mkdir -p $D
H="/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -fPIC -std=c++17 -Wall -Iinclude -I$C"
$H $FLAGS -c $C/bt_kernels.hip -o $D/bt_kernels.o
g++ -O2 -fPIC -std=c++17 -Wall -Iinclude -I$C $RING_FLAGS -c $C/bt_ring.cpp -o $D/bt_ring.o
REST=$(make -s --no-print-directory -C $C print-objs | grep -v -e '/bt_kernels\.o$' -e '/bt_ring\.o$' | sed "s|^|$C/|")
$H -shared -fPIC -o $D/libbeatrice_gpu.so $D/bt_kernels.o $D/bt_ring.o $REST
rm -f $D/bt_kernels.o $D/bt_ring.o
echo built $D
