# host/tests/map_fuse.mk -- test_map_fuse: the mirror of the fusion of duplicate map points (my_slam/vo/map_fuse.h), written
# against the reference-shaped headers and linked to libmvo_hip.so only (tests/test_map_fuse_host.py runs it on the MI355X and,
# with the emulated build in front of the library search path, on the CPU).
#   make -C host/tests -f map_fuse.mk
include Makefile
map_fuse: test_map_fuse
test_map_fuse: test_map_fuse.cpp $(DROPIN) $(wildcard ../include/my_slam/*.h ../include/my_slam/*/*.h) $(ROOT)/include/mvo_hip.h
	$(CXX) $(CXXFLAGS) -o $@ test_map_fuse.cpp $(DROPIN) -L$(LIBDIR) -lmvo_hip -Wl,-rpath,'$$ORIGIN/../../csrc' -Wl,-rpath,/opt/rocm/lib
.DEFAULT_GOAL := map_fuse
.PHONY: map_fuse
