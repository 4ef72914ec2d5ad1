# tests/sim/epipolar.mk -- TEST AID built by tests/test_epipolar_sim.py into tests/sim/_build/ (never part of
# libmvo_hip.so): libmvo_sim_epipolar.so = the objects of libmvo_sim_undistort.so (undistort.mk) plus
# csrc/epipolar_host.cpp and csrc/epipolar_kernels.hip, compiled for x86 against hip_emu/ by the same pattern rule: every
# lane of k_knn2_epipolar runs as a fiber on the CPU.
#   make -C tests/sim -f epipolar.mk _build/libmvo_sim_epipolar.so
include undistort.mk
_build/libmvo_sim_epipolar.so: $(FULL_OBJ) _build/full/init_host.cpp.o _build/full/undistort_host.cpp.o _build/full/undistort_kernels.hip.o _build/full/epipolar_host.cpp.o _build/full/epipolar_kernels.hip.o
	$(CXX) -shared -fPIC -pthread -o $@ $^
