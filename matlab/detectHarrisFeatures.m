function points = detectHarrisFeatures(I, varargin)
%detectHarrisFeatures  Harris-Stephens corners on the GPU through vo_mex('corners', ...).
%   points = detectHarrisFeatures(I, MinQuality = q, FilterSize = f, ROI = [x y w h]) shadows the toolbox
%   function of the same name when this folder is ahead of it on the path and returns
%   cornerPoints(Location, "Metric", Metric).  I is a uint8 grey image (another class is converted with
%   im2uint8).  The response is det - 0.04 trace^2 of the smoothed gradient matrix detectMinEigenFeatures
%   takes the smaller eigenvalue of (DESIGN.md 3.5.4).
p = inputParser;
addParameter(p, 'MinQuality', 0.01, @(v) isscalar(v) && isreal(v));
addParameter(p, 'FilterSize', 5, @(v) isscalar(v) && isreal(v));
addParameter(p, 'ROI', [0 0 0 0], @(v) isnumeric(v) && numel(v) == 4);
parse(p, varargin{:});
if ~isa(I, 'uint8'), I = im2uint8(I); end
roi = double(p.Results.ROI(:)');
opts = [1, double(p.Results.FilterSize), double(p.Results.MinQuality), 0, roi];
[Location, Metric] = vo_mex('corners', I, opts);
points = cornerPoints(Location, "Metric", Metric);
end
