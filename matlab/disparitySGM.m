function disparityMap = disparitySGM(I1, I2, varargin)
%disparitySGM  Semi-global matching on the GPU through vo_mex('disparitysgm', ...).
%   disparityMap = disparitySGM(I1, I2, DisparityRange = [min max], UniquenessThreshold = u) shadows the toolbox
%   function of the same name when this folder is ahead of it on the path.  I1, I2 are the rectified left and
%   right uint8 grey images (another class is converted with im2uint8); max - min is divisible by 8 and at most
%   128.  disparityMap is single, NaN where the match is unreliable or falls outside I2.  The spec is libvo's
%   (DESIGN.md 3.5.5): census cost, eight paths, the toolbox's uniqueness rule; any other option is refused by name.
p = inputParser;
p.FunctionName = 'disparitySGM';
addParameter(p, 'DisparityRange', [0 128], @(v) isnumeric(v) && isreal(v) && numel(v) == 2);
addParameter(p, 'UniquenessThreshold', 15, @(v) isscalar(v) && isreal(v));
parse(p, varargin{:});
if ~isa(I1, 'uint8'), I1 = im2uint8(I1); end
if ~isa(I2, 'uint8'), I2 = im2uint8(I2); end
r = double(p.Results.DisparityRange(:)');
disparityMap = vo_mex('disparitysgm', I1, I2, [r, double(p.Results.UniquenessThreshold)]);
end
