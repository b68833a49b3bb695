# tests/cpp/sddmm_sim.mk — TEST CODE.  sddmm_sim: csrc/sddmm.hip compiled UNCHANGED with the host compiler over simt/
# (a stand-in hip_runtime.h that runs every lane as a fiber), with the address and undefined-behaviour sanitizers, and
# driven through mi355_spmv_sddmm_*.  Built on demand by tests/test_sddmm_sim_cpu.py with the flags of the other host
# simulations (tests/cpp/Makefile, SIM_SAN):   make -C tests/cpp -f sddmm_sim.mk sddmm_sim
CXX      ?= g++
CSRC     := ../../spmv-samples_amd/csrc
# the sanitizer runtimes are linked statically: the program then loads the same way whatever the environment preloads
SIM_SAN  ?= -fsanitize=address,undefined -fno-sanitize-recover=undefined -static-libasan -static-libubsan

sddmm_sim: sddmm_sim.cpp simt/hip/hip_runtime.h sim_io.hpp $(CSRC)/sddmm.hip $(CSRC)/slice_cut.hpp \
           $(CSRC)/slice_cut.inc $(CSRC)/slice_cut_row.inc $(CSRC)/common.hpp ../../include/mi355_spmv.h
	$(CXX) -std=c++17 -O1 -g -fno-omit-frame-pointer $(SIM_SAN) -Isimt -o $@ $<

clean:
	rm -f sddmm_sim
.PHONY: clean
