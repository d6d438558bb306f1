// table_images.hpp — the host-built table images (table_images.cpp), for
// api.cpp's device context and the host checks under tests/cpp.
#pragma once
#include <cstdint>
#include <vector>

namespace lnx {

std::vector<uint32_t> build_lds_image(uint32_t rl);     // lds_layout.hpp: the 160 KiB rows image of row width rl
const std::vector<uint32_t>& host_image();              // the rows images, compact, back to back (image_index)
std::vector<uint32_t> build_stage_image();              // table_layout.hpp: kStageImageDwords
std::vector<uint32_t> build_rx_image();                 // kRxImageDwords
std::vector<uint32_t> build_search_tables();            // kSearchTableDwords
std::vector<uint32_t> build_rst_image();                // kRstImageDwords
std::vector<uint32_t> build_echo_image();               // kEchoImageDwords

}  // namespace lnx
