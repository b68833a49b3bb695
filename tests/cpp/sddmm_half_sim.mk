# tests/cpp/sddmm_half_sim.mk — TEST CODE.  sddmm_half_sim: csrc/sddmm.hip with csrc/sddmm_half_kernel.hpp, which it
# includes, compiled UNCHANGED with the host compiler over simt/ (a stand-in hip_runtime.h that runs every lane as a
# fiber), with the address and undefined-behaviour sanitizers, and driven through mi355_spmv_sddmm_create_half and the
# object's entry points.  A stand-alone program, built on demand by tests/test_sddmm_half_sim_cpu.py exactly as
# sddmm_sim.mk builds sddmm_sim:   make -C tests/cpp -f sddmm_half_sim.mk sddmm_half_sim
CXX      ?= g++
CSRC     := ../../spmv-samples_amd/csrc
# the sanitizer runtimes are linked statically: the program then loads the same way whatever the environment preloads
SIM_SAN  ?= -fsanitize=address,undefined -fno-sanitize-recover=undefined -static-libasan -static-libubsan

sddmm_half_sim: sddmm_half_sim.cpp simt/hip/hip_runtime.h sim_io.hpp $(CSRC)/sddmm.hip $(CSRC)/sddmm_half_kernel.hpp \
                $(CSRC)/half_cols.hpp $(CSRC)/half_convert.hpp $(CSRC)/slice_cut.hpp $(CSRC)/slice_cut.inc \
                $(CSRC)/slice_cut_row.inc $(CSRC)/common.hpp ../../include/mi355_spmv.h
	$(CXX) -std=c++17 -O1 -g -fno-omit-frame-pointer $(SIM_SAN) -Isimt -o $@ $<

clean:
	rm -f sddmm_half_sim
.PHONY: clean
